"""Sentence CNN encoder (reference: module/Encoder.py:18-76).

Not part of the WSWGAT hot path but in the logits path and the
next row of SURVEY §8f (rank 3).  Same parameter layout as the reference
(``ngram_enc.{embed,position_embedding,convs.0-5}``), so state_dicts load unchanged.
Differences in *how*: no Python loop over sentences for the positions
(Encoder.py:60-66), and the six convolutions + ReLU + max-pool run as one MFMA GEMM
over the sentences' real rows plus the HIP gather / pool kernels
(:mod:`hetersumgraph_amd.cnn`, hsg_cnn.hip).  There is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.init as init

from .. import cnn as _cnn
from ..cnn import sent_cnn_mode, sent_cnn_rows, sent_cnn_switched, token_path_ok
from .PositionEmbedding import get_sinusoid_encoding_table

WORD_PAD = "[PAD]"


class sentEncoder(nn.Module):
    def __init__(self, hps, embed):
        super().__init__()
        self._hps = hps
        self.sent_max_len = hps.sent_max_len
        width = hps.word_emb_dim
        self.embed = embed
        self.position_embedding = nn.Embedding.from_pretrained(
            get_sinusoid_encoding_table(self.sent_max_len + 1, width, padding_idx=0), freeze=True)
        # kernel heights 2..7, 50 channels each -> 300-d (Encoder.py:36-53)
        self.convs = nn.ModuleList([nn.Conv2d(1, 50, kernel_size=(kh, width)) for kh in range(2, 8)])
        for conv in self.convs:
            init.xavier_normal_(conv.weight.data, gain=np.sqrt(6.0))
        # the vocabulary product table of the inference path (HSG_SENT_CNN_VOCAB): not a parameter,
        # not a buffer, never in a state_dict
        self._vocab_table = _cnn.VocabTable()

    def _vocab_args(self):
        return (self.embed.weight, self.position_embedding.weight, [c.weight for c in self.convs],
                [c.bias for c in self.convs])

    def _takes_vocab_path(self, input):
        return _cnn.sent_cnn_vocab_on() and not self.training and _cnn.vocab_path_ok(input, *self._vocab_args())

    def drop_vocab_table(self):
        """Forget the vocabulary product table: the next no-grad forward builds a fresh one.  For a
        parameter write the table's key cannot see (``.data``, a foreign kernel) inside one
        ``eval()`` span."""
        self._vocab_table.drop()

    def train(self, mode=True):
        # every model.train() / model.eval() starts a fresh table
        self._vocab_table.drop()
        return super().train(mode)

    def forward(self, input, layout=None):
        # input: [n_sent, L] token ids, PAD = 0 (trailing) -> [n_sent, 300]
        # Opt-in (``path_options(HSG_SENT_CNN="dw" | "tokens")``): with a frozen
        # embedding, the sparse weight gradient / the forward on the batch's distinct tokens.
        # ``layout``: the sentences' prebuilt row layout (cnn.BatchLayout) instead of the one
        # computed, and read back, from ``input``
        # Opt-in (``path_options(HSG_SENT_CNN_VOCAB="1")``): in eval mode, when no gradient is
        # recorded, one gather launch on the vocabulary product table
        if self._takes_vocab_path(input):
            emb, pos, cw, cb = self._vocab_args()
            return _cnn.sent_cnn_vocab(input, self._vocab_table.get(emb, pos, cw), cb, layout=layout)
        return sent_cnn_switched(input, self.embed.weight, self.position_embedding.weight,
                                 [c.weight for c in self.convs], [c.bias for c in self.convs],
                                 padding_idx=getattr(self.embed, "padding_idx", None), layout=layout)

    def takes_token_path(self, input):
        """True when :meth:`forward` would run ``input`` on a token path (``HSG_SENT_CNN``) or on
        the vocabulary path (``HSG_SENT_CNN_VOCAB``): the encoder then reads the ids itself."""
        if self._takes_vocab_path(input):
            return True
        return sent_cnn_mode() != "0" and token_path_ok(input, self.embed.weight, self.position_embedding.weight)

    def forward_rows(self, X, layout, shape):
        """:meth:`forward` from the gathered row matrix on (``X``, ``layout`` from
        :func:`hetersumgraph_amd.wordembed.embed_batch` for ids of ``shape``)."""
        return sent_cnn_rows(X, layout, shape, [c.weight for c in self.convs], [c.bias for c in self.convs])
