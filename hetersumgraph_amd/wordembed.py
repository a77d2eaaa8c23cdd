"""The trainable word embedding on the native path (hsg_embed.hip, include/hsg_embed.h).

``train.py --embed_train`` (train.py:342) lets the shared ``nn.Embedding`` train.  The
model reads it in two places -- the word nodes (HiGraph.py:144-152) and the sentence CNN's
rows (module/Encoder.py:56-68) -- so :func:`embed_batch` makes BOTH lookups one autograd
node: its backward receives the two row gradients together and runs one deterministic
reduce (``hsg_embed_grad``) into one dense ``[V, D]`` gradient.  No float atomics: the sum
of a token's rows follows the order contract of hsg_embed.h, a function of positions in
the sorted occurrence list alone, so a training step stays bitwise reproducible.

The occurrence plan (the sorted ``(token, source row)`` keys) is built per forward, on the
device, from ``wid`` and ``ids`` only: it holds indices, never weights, so nothing in it
goes stale after ``optimizer.step()``.  With a frozen table neither the sort nor the
reduce runs.  Parameters stay in the ``nn.Embedding`` module.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import check, load, ptr, stream_of
from .cnn import _layout

DROPPED = torch.iinfo(torch.int64).max     # key of a dropped occurrence: sorts behind every kept one


def embed_supported(D: int) -> bool:
    return bool(load().hsg_embed_supported(int(D)))


def native_embed_ok(embed, encoder) -> bool:
    """The native path covers this model: a plain fp32 ``nn.Embedding`` on a ROCm device
    whose width ``hsg_embed_supported`` takes, shared with the sentence encoder."""
    if not isinstance(embed, nn.Embedding) or getattr(encoder, "embed", None) is not embed:
        return False
    if embed.max_norm is not None or embed.scale_grad_by_freq or embed.sparse:
        return False
    w = embed.weight
    return w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and embed_supported(w.shape[1])


def occurrence_keys(wid, ids, rowoff, rows, padding_idx):
    """Sorted int64 keys ``token << 32 | source`` of every occurrence (hsg_embed.h): the
    word rows are sources ``[0, n_w)``, CNN row ``r`` is source ``n_w + r`` with the token
    of its position, 0 for a sentence's pad row.  Occurrences of ``padding_idx`` get the
    key DROPPED.  ``n_w + rows`` entries: one launch and one sort, no host readback."""
    n_w = wid.shape[0]
    n, L = ids.shape
    keys = torch.empty(n_w + rows, dtype=torch.int64, device=wid.device)
    check(load().hsg_embed_keys(n_w, n, L, rows, ptr(wid), ptr(ids), ptr(rowoff), -1 if padding_idx is None else padding_idx,
                                ptr(keys), stream_of(wid)), "hsg_embed_keys")
    return torch.sort(keys).values


def _rows_operand(g, D):
    """A row gradient as the kernel reads it: unit column stride, pitch a multiple of 4,
    16-byte aligned base (anything else is copied once)."""
    if g.stride(1) != 1 or g.stride(0) < D or g.stride(0) % 4 or g.data_ptr() % 16:
        g = g.contiguous()
    return g


def embed_grad(keys, n_occ, V, D, dW, dX):
    """``hsg_embed_grad`` on sorted ``keys``: dense ``[V, D]`` gradient of the rows ``dW``
    (sources ``[0, n_w)``) and ``dX`` (sources from ``n_w``); either may be None."""
    lib = load()
    ref = dW if dW is not None else dX
    dE = torch.empty(V, D, dtype=torch.float32, device=keys.device)
    n_ws = lib.hsg_embed_ws_floats(n_occ, D)
    ws = torch.empty(n_ws, dtype=torch.float32, device=keys.device) if n_ws else None
    dW = _rows_operand(dW, D) if dW is not None and dW.shape[0] else None
    dX = _rows_operand(dX, D) if dX is not None and dX.shape[0] else None
    check(lib.hsg_embed_grad(V, D, n_occ, ptr(keys), 0 if dW is None else dW.shape[0], ptr(dW),
                             0 if dW is None else dW.stride(0), 0 if dX is None else dX.shape[0], ptr(dX),
                             0 if dX is None else dX.stride(0), ptr(dE), ptr(ws),
                             stream_of(ref if ref is not None else dE)), "hsg_embed_grad")
    return dE


class _EmbedBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, wid, ids, pos_w, padding_idx, rowoff, rows):
        lib = load()
        V, D = weight.shape
        n_w = wid.shape[0]
        n, L = ids.shape
        st = stream_of(weight)
        Xw = weight.new_empty(n_w, D)
        check(lib.hsg_embed_rows(n_w, V, D, ptr(wid), ptr(weight), ptr(Xw), D, st), "hsg_embed_rows")
        X = weight.new_empty(rows, D)
        if rows:
            check(lib.hsg_cnn_gather(n, L, D, ptr(ids), ptr(weight), ptr(pos_w), ptr(rowoff), rows, ptr(X), st),
                  "hsg_cnn_gather")
        ctx.set_materialize_grads(False)             # an unused output arrives as None, not as zeros
        ctx.shape, ctx.n_w, ctx.rows = (V, D), n_w, rows
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(occurrence_keys(wid, ids, rowoff, rows, padding_idx))
        return Xw, X

    @staticmethod
    def backward(ctx, dW, dX):
        if not ctx.needs_input_grad[0] or (dW is None and dX is None):
            return (None,) * 7
        (keys,) = ctx.saved_tensors
        V, D = ctx.shape
        n_w = ctx.n_w
        if dW is None or dX is None:
            # one side only: the other has no occurrences.  Drop its keys and sort again, so
            # that list positions (the order contract) are those of the remaining side alone.
            src = keys & 0xFFFFFFFF
            if dW is None:
                keys = torch.where((src >= n_w) & (keys != DROPPED), keys - n_w, torch.full_like(keys, DROPPED))
            else:
                keys = torch.where(src < n_w, keys, torch.full_like(keys, DROPPED))
            keys = torch.sort(keys).values
        dE = embed_grad(keys, keys.shape[0], V, D, dW, dX)
        return (dE,) + (None,) * 6


def embed_batch(weight, wid, ids, pos_weight, padding_idx, layout=None):
    """Both lookups of one batch as ONE autograd node over ``weight [V, D]``:

    * ``w_embed [n_w, D] = weight[wid]`` (``hsg_embed_rows``; bitwise ``F.embedding``);
    * ``X [rows, D]``, the sentence CNN's row matrix of ``ids [n, L]`` (``hsg_cnn_gather``
      over the layout :func:`hetersumgraph_amd.cnn._layout` gives: each sentence's real
      rows ``weight[ids] + pos_weight[t + 1]`` and one pad row ``weight[0] + pos_weight[0]``).

    Returns ``(w_embed, X, (length, rowoff, rows))``; the layout goes on to
    :func:`hetersumgraph_amd.cnn.sent_cnn_rows`.  The backward sums ``dW`` and ``dX`` into
    one dense gradient in the fixed order of hsg_embed.h; row ``padding_idx`` (if not None)
    is exactly zero, as ``nn.Embedding(padding_idx=...)``.  ``layout``: a prebuilt
    :class:`hetersumgraph_amd.cnn.BatchLayout` of ``ids`` in place of the one computed here."""
    if not weight.is_cuda or weight.dtype != torch.float32:
        raise RuntimeError("hetersumgraph_amd word embedding runs only on a ROCm device in fp32 (no CPU fallback)")
    if not embed_supported(weight.shape[1]):
        raise ValueError(f"word embedding: width {weight.shape[1]} is not a multiple of 4 in the supported range")
    wid = wid.long().contiguous()
    ids = ids.long().contiguous()
    length, rowoff, rows = _layout(ids) if layout is None else layout.check(ids)
    w_embed, X = _EmbedBatch.apply(weight.contiguous(), wid, ids, pos_weight.contiguous(), padding_idx, rowoff, rows)
    return w_embed, X, (length, rowoff, rows)
