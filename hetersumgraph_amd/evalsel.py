"""Evaluation-time sentence selection on the native kernel (C ABI: hsg_eval_select,
include/hsg_eval.h, csrc/hsg_eval.hip).

Reference: ``SLTester.evaluation`` (Tester.py:105-140) and ``ngram_blocking``
(Tester.py:155-184).  The device does the candidate order, the top-m walk with or without
n-gram blocking, the m == 0 rule and the four match counters in one launch per batch.  The
host's part of blocking is to turn every distinct n-gram of a document into a dense
document-local integer id (:func:`ngram_ids`, :func:`pack_batch`), so that "shares an n-gram
with a chosen sentence" is a bitmap test on the device: no string reaches it.

There is no fallback: tensors that are not on a ROCm device, or a batch beyond the limits
of ``hsg_eval_select_supported``, raise ``RuntimeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, load, ptr, stream_of


def _require(cond, what):
    if not cond:
        raise RuntimeError(f"evalsel: {what} (no fallback)")


def ngram_ids(sents, n_win, n_rows=None):
    """(ptr int32 [N + 1], ids int32 [T], n_distinct): the ids of sentence i are
    ``ids[ptr[i]:ptr[i + 1]]``, dense in [0, n_distinct) and local to this document.

    Pieces are ``s.split()`` (Python's own split, so Unicode whitespace behaves as in the
    reference); the windows of a sentence are ``range(len(pieces) - n_win)`` -- the reference
    never uses a sentence's last n-gram (Tester.py:167).  Words are interned through a dict
    and the window rows made dense with one ``np.unique``; pieces contain no whitespace, so
    equal id tuples are exactly equal joined strings.  ``n_rows`` (default ``len(sents)``) is
    the number of sentence nodes: sentences beyond it are not looked at, rows beyond the
    article get no ids."""
    N = len(sents) if n_rows is None else int(n_rows)
    words, flat = {}, []
    lens = np.zeros(N, np.int64)
    for i, s in enumerate(sents[:N]):
        w = [words.setdefault(p, len(words)) for p in s.split()]
        flat += w
        lens[i] = len(w)
    c = np.maximum(lens - n_win, 0)                       # windows per sentence
    ptr_ = np.zeros(N + 1, np.int32)
    np.cumsum(c, out=ptr_[1:])
    T = int(ptr_[-1])
    if T == 0:
        return ptr_, np.zeros(0, np.int32), 0
    # window t of the document starts at flat position first[t]: all sentences at once
    first = np.repeat(np.cumsum(lens) - lens - ptr_[:-1], c) + np.arange(T)
    rows = np.asarray(flat, np.int64)[first[:, None] + np.arange(n_win)]
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    return ptr_, inv.reshape(-1).astype(np.int32), int(uniq.shape[0])


class GramPack:
    """One batch's blocking operands in ONE int32 buffer: [gram_ptr (n + 1) | gram_cnt (B) |
    gram_ids (T, at least one element so that its pointer is never NULL)]."""

    def __init__(self, buf, n, B, T, gram_max):
        self.buf, self.n, self.B, self.T, self.gram_max = buf, n, B, T, gram_max

    def views(self, buf=None):
        """(gram_ptr, gram_ids, gram_cnt) as views of ``buf`` (default: the host buffer)."""
        buf = self.buf if buf is None else buf
        a, b = self.n + 1, self.n + 1 + self.B
        return buf[:a], buf[b:], buf[a:b]

    def to(self, device):
        """The device copy (one non-blocking copy when the host buffer is pinned)."""
        return GramPack(self.buf.to(device, non_blocking=True), self.n, self.B, self.T, self.gram_max)


def pack_batch(list_of_sents, counts, n_win, pin=None):
    """:class:`GramPack` of a batch: ``list_of_sents[d]`` are document d's article sentences,
    ``counts[d]`` its number of sentence nodes.  The buffer is pinned when a GPU is present
    (``pin``), so that :meth:`GramPack.to` is one asynchronous copy."""
    B, n = len(counts), int(sum(counts))
    parts = [ngram_ids(s, n_win, c) for s, c in zip(list_of_sents, counts)]
    T = sum(len(p[1]) for p in parts)
    pin = torch.cuda.is_available() if pin is None else pin
    buf = torch.empty(n + 1 + B + max(T, 1), dtype=torch.int32, pin_memory=pin)
    a = buf.numpy()
    a[n + 1 + B:] = 0
    row, t = 0, 0
    a[0] = 0
    for d, (p, ids, cnt) in enumerate(parts):
        a[row + 1:row + 1 + counts[d]] = p[1:] + t
        a[n + 1 + d] = cnt
        a[n + 1 + B + t:n + 1 + B + t + len(ids)] = ids
        row += counts[d]
        t += len(ids)
    return GramPack(buf, n, B, T, max([p[2] for p in parts], default=0))


def supported(n_max, gram_max=0):
    return bool(load().hsg_eval_select_supported(int(n_max), int(gram_max)))


def select(logits, labels, doc_off, m, n_max, totals, grams=None, sel_ld=None, out=None):
    """``hsg_eval_select`` on device tensors: returns (sel int32 [B, sel_ld], nsel int32 [B],
    doc_counts int32 [B, 4]) and adds the batch's counters into ``totals`` (int64 [4], on the
    device, accumulated).  ``grams``: a device :class:`GramPack` for n-gram blocking, or
    None.  ``out``: optional (sel, nsel, doc_counts) to write into.  Nothing here waits for
    the device."""
    _require(torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32,
             "logits must be fp32 on a ROCm device")
    _require(logits.dim() == 2 and logits.shape[1] == 2, "logits must be [n, 2]")
    dev, n = logits.device, logits.shape[0]
    for name, t, dt in (("labels", labels, torch.int64), ("doc_off", doc_off, torch.int32),
                        ("totals", totals, torch.int64)):
        _require(torch.is_tensor(t) and t.device == dev and t.dtype == dt and t.is_contiguous(),
                 f"{name} must be contiguous {dt} on the logits' device")
    _require(labels.shape == (n,), "labels must be [n]")
    _require(doc_off.dim() == 1 and doc_off.numel() >= 2, "doc_off must be [B + 1] with B >= 1")
    _require(totals.shape == (4,), "totals must be [4]")
    B, m, n_max = doc_off.numel() - 1, int(m), int(n_max)
    _require(m >= 0, "m must be >= 0")
    gram_max = 0
    gp = gi = gc = None
    if grams is not None:
        _require(grams.buf.device == dev and grams.buf.dtype == torch.int32 and grams.buf.is_contiguous(),
                 "the gram pack must be int32 on the logits' device")
        _require(grams.n == n and grams.B == B, "the gram pack is of another batch")
        gp, gi, gc = grams.views()
        gram_max = int(grams.gram_max)
    _require(supported(n_max, gram_max),
             f"n_max {n_max} / gram_max {gram_max} beyond hsg_eval_select_supported (1..1024 rows, 0..262144 n-grams)")
    need = n_max if m == 0 else min(m, n_max)
    sel_ld = need if sel_ld is None else int(sel_ld)
    _require(sel_ld >= need, f"sel_ld {sel_ld} below {need}")
    if out is None:
        out = (torch.empty(B, sel_ld, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, 4, dtype=torch.int32, device=dev))
    sel, nsel, doc_counts = out
    for name, t, shape in (("sel", sel, (B, sel_ld)), ("nsel", nsel, (B,)), ("doc_counts", doc_counts, (B, 4))):
        _require(t.device == dev and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape,
                 f"{name} must be contiguous int32 {shape} on the logits' device")
    logits = logits.contiguous()
    check(load().hsg_eval_select(n, B, ptr(logits), ptr(labels), ptr(doc_off), m, n_max, ptr(gp), ptr(gi), ptr(gc),
                                 gram_max, ptr(sel), sel_ld, ptr(nsel), ptr(doc_counts), ptr(totals),
                                 stream_of(logits)), "hsg_eval_select")
    return sel, nsel, doc_counts
