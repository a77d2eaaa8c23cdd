"""The training loss of train.py:115-119 on the native kernel (C ABI: hsg_doc_ce,
include/hsg_train.h, csrc/hsg_train.hip).

Reference: ``criterion(outputs, label)`` per sentence (CrossEntropyLoss, reduction
'none'), written into the node column ``loss``, ``dgl.sum_nodes`` per document and
``mean`` over the batch.  :func:`doc_mean_cross_entropy` computes the same scalar in two
launches -- a block per document, then a one-block finish -- as ONE autograd node whose
backward is the saved ``(softmax - onehot) / B`` times the incoming gradient.  Every sum
runs in a fixed order, so the loss and its gradient are bitwise reproducible.

There is no fallback: logits that are not fp32 on a ROCm device raise ``RuntimeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, load, ptr, stream_of


def _require(cond, what):
    if not cond:
        raise RuntimeError(f"doc_mean_cross_entropy: {what} (no fallback)")


class _DocCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, doc_off, rows):
        n, C = logits.shape
        B = doc_off.numel() - 1
        row_loss = logits.new_empty(n)
        doc_loss = logits.new_empty(B)
        mean = logits.new_empty(())
        dlogits = torch.empty_like(logits)
        if rows is None:
            L, N = 1, labels.shape[0]
        else:
            N, L = labels.shape
        check(load().hsg_doc_ce(n, C, B, ptr(logits), ptr(labels), L, N, ptr(rows), ptr(doc_off), ptr(row_loss),
                                ptr(doc_loss), ptr(mean), ptr(dlogits), stream_of(logits)), "hsg_doc_ce")
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(doc_loss, row_loss)
        return mean, doc_loss, row_loss

    @staticmethod
    def backward(ctx, dmean, _ddoc, _drow):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dmean, None, None, None


def doc_cross_entropy(logits, labels, doc_off, rows=None):
    """(mean over documents, per-document sums [B], per-row losses [n]) of the cross
    entropy of ``logits`` [n, 2]; only the mean carries a gradient.

    ``labels``: int64 [n] classes, or with ``rows`` (int64 [n] node ids) the node label
    matrix int64 [N, L], the class of row i being ``labels[rows[i]].sum()`` (train.py:116).
    ``doc_off``: int32 [B + 1] row offsets of the documents (an empty document adds 0).  A
    label outside {0, 1} makes that row's loss -- and so the mean -- NaN and its gradient
    row zero."""
    _require(torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32,
             "logits must be fp32 on a ROCm device")
    _require(logits.dim() == 2 and logits.shape[1] == 2, "logits must be [n, 2]")
    n = logits.shape[0]
    for name, t, dt in (("labels", labels, torch.int64), ("doc_off", doc_off, torch.int32), ("rows", rows, torch.int64)):
        if t is None and name == "rows":
            continue
        _require(torch.is_tensor(t) and t.device == logits.device and t.dtype == dt,
                 f"{name} must be {dt} on the logits' device")
    _require(doc_off.dim() == 1 and doc_off.numel() >= 2, "doc_off must be [B + 1] with B >= 1")
    if rows is None:
        _require(labels.dim() == 1 and labels.shape[0] == n, "labels must be [n]")
    else:
        _require(labels.dim() == 2 and rows.dim() == 1 and rows.shape[0] == n,
                 "labels must be [N, L] and rows [n]")
        rows = rows.contiguous()
    return _DocCE.apply(logits.contiguous(), labels.contiguous(), doc_off.contiguous(), rows)


def doc_mean_cross_entropy(logits, labels, doc_off, rows=None):
    """The scalar of train.py:117-119: per-row cross entropy, summed per document,
    averaged over the documents (see :func:`doc_cross_entropy`)."""
    return doc_cross_entropy(logits, labels, doc_off, rows)[0]


def sentence_loss_inputs(G):
    """(rows, labels, doc_off) of a batch: the sentence node ids (ascending, train.py:115),
    the node label matrix, and the int32 [B + 1] row offsets of the member graphs'
    sentences -- sentence rows are contiguous per member graph, for HSG and HDSG alike.
    The offsets are built once per graph and cached on it."""
    from . import HiGraph
    rows = HiGraph.node_ids(G, "dtype", 1.0)

    def build():
        counts = HiGraph.sentence_counts(G)
        off = np.zeros(len(counts) + 1, np.int32)
        off[1:] = np.cumsum(counts)
        return torch.from_numpy(off).to(G.device)
    return rows, G.ndata["label"], HiGraph._cached(G, "sent_doc_off", build)


def sentence_loss(G, outputs, keep_node_loss=False):
    """What train.py:115-119 computes from the model's ``outputs`` [n_sent, 2]: the mean
    over the batch's documents of their summed sentence cross entropies.  The node column
    ``G.ndata['loss']`` of the reference is written only with ``keep_node_loss``."""
    rows, labels, doc_off = sentence_loss_inputs(G)
    mean, _, row_loss = doc_cross_entropy(outputs, labels, doc_off, rows)
    if keep_node_loss:
        G.nodes[rows].data["loss"] = row_loss.unsqueeze(-1)
    return mean
