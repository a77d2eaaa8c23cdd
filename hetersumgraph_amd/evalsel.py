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

The second half of the module is the same selection with blocking on WORD ids
(``hsg_eval_select_words``, include/hsg_eval_words.h): :func:`word_ids`, :func:`pack_words`,
:func:`select_words` and the per-example cache :func:`words_for`.
"""
from __future__ import annotations

import weakref

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


# ---- blocking on word ids (C ABI: hsg_eval_select_words, include/hsg_eval_words.h) ----------
# The device forms the n-gram windows itself and keeps the chosen sentences' windows in a hash
# set in LDS, so the host's part is the words' document-local ids alone.  They depend neither
# on the window length nor on m: the dataset can attach them to the graph in the DataLoader
# workers (``ExampleSet(eval_words=True)``), and :func:`words_for` keeps them per example.

def word_ids(sents, n_rows=None):
    """(ptr int32 [N + 1], ids int32 [W]): the words of sentence i are ``ids[ptr[i]:ptr[i + 1]]``.

    Pieces are ``s.split()`` (Python's own split, as the reference's), interned through one
    dict per document in first-appearance order: equal id <=> equal piece.  ``n_rows``
    (default ``len(sents)``) is the number of sentence nodes: sentences beyond it are not
    looked at, rows beyond the article are empty."""
    N = len(sents) if n_rows is None else int(n_rows)
    words, flat = {}, []
    ptr_ = np.zeros(N + 1, np.int32)
    for i, s in enumerate(sents[:N]):
        flat += [words.setdefault(p, len(words)) for p in s.split()]
        ptr_[i + 1] = len(flat)
    ptr_[len(sents[:N]) + 1:] = len(flat)
    return ptr_, np.asarray(flat, np.int32)


def _next_pow2(x):
    return 1 << max(int(x) - 1, 0).bit_length()


class WordPack:
    """One batch's blocking operands in ONE int32 buffer: [word_ptr (n + 1) | word_ids (W, at
    least one element so that its pointer is never NULL)].  ``lens`` (words per row) and
    ``counts`` (rows per document) stay on the host for :meth:`tab_cap`."""

    def __init__(self, buf, n, B, W, lens, counts):
        self.buf, self.n, self.B, self.W, self.lens, self.counts = buf, n, B, W, lens, counts

    def views(self, buf=None):
        """(word_ptr, word_ids) as views of ``buf`` (default: this pack's buffer)."""
        buf = self.buf if buf is None else buf
        return buf[:self.n + 1], buf[self.n + 1:]

    def to(self, device):
        """The device copy (one non-blocking copy when the host buffer is pinned)."""
        return WordPack(self.buf.to(device, non_blocking=True), self.n, self.B, self.W, self.lens, self.counts)

    def win_need(self, n_win, m):
        """The most windows a document of the batch can have stored: over the documents, the
        largest sum of the min(m, N_d) largest per-sentence window counts (with repeats)."""
        win = np.maximum(self.lens - int(n_win), 0)
        need, o = 0, 0
        for c in self.counts:
            k = min(int(m), c)
            if k > 0:
                need = max(need, int(np.sort(win[o:o + c])[c - k:].sum()))
            o += c
        return need

    def tab_cap(self, n_win, m):
        """Slots of the device's seen set for this batch: max(64, next_pow2(2 * win_need)), a
        load of at most one half whichever sentences are chosen."""
        return max(64, _next_pow2(2 * self.win_need(n_win, m)))


def pack_words(parts, counts, pin=None):
    """:class:`WordPack` of a batch: ``parts[d]`` is document d's ``(ptr, ids)`` of
    :func:`word_ids` for its ``counts[d]`` sentence nodes.  The buffer is pinned when a GPU is
    present (``pin``), so that :meth:`WordPack.to` is one asynchronous copy."""
    counts = [int(c) for c in counts]
    B, n = len(counts), sum(counts)
    _require(len(parts) == B and all(len(p[0]) == c + 1 for p, c in zip(parts, counts)),
             "word ids and sentence counts are of different batches")
    W = sum(len(p[1]) for p in parts)
    pin = torch.cuda.is_available() if pin is None else pin
    buf = torch.empty(n + 1 + max(W, 1), dtype=torch.int32, pin_memory=pin)
    a = buf.numpy()
    a[n + 1:] = 0
    a[0] = 0
    row, w = 0, 0
    for (p, ids), c in zip(parts, counts):
        a[row + 1:row + 1 + c] = p[1:] + w
        a[n + 1 + w:n + 1 + w + len(ids)] = ids
        row += c
        w += len(ids)
    return WordPack(buf, n, B, W, np.diff(a[:n + 1]).astype(np.int64), counts)


def words_supported(n_max, n_win=1, tab_cap=64):
    return bool(load().hsg_eval_words_supported(int(n_max), int(n_win), int(tab_cap)))


def select_words(logits, labels, doc_off, m, n_max, n_win, totals, words=None, tab_cap=None, sel_ld=None, out=None):
    """``hsg_eval_select_words`` on device tensors: returns (sel int32 [B, sel_ld], nsel int32
    [B], doc_counts int32 [B, 4]) and adds the batch's counters into ``totals`` (int64 [4], on
    the device, accumulated).  ``words``: a device :class:`WordPack` for n-gram blocking with
    windows of ``n_win`` words, or None.  ``tab_cap`` defaults to the pack's own rule.
    ``out``: optional (sel, nsel, doc_counts) to write into.  Nothing here waits for the
    device."""
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
    B, m, n_max, n_win = doc_off.numel() - 1, int(m), int(n_max), int(n_win)
    _require(m >= 0, "m must be >= 0")
    wp = wi = None
    if words is not None:
        _require(words.buf.device == dev and words.buf.dtype == torch.int32 and words.buf.is_contiguous(),
                 "the word pack must be int32 on the logits' device")
        _require(words.n == n and words.B == B, "the word pack is of another batch")
        wp, wi = words.views()
    if tab_cap is None:
        tab_cap = 64 if words is None else words.tab_cap(n_win, m)
    tab_cap = int(tab_cap)
    _require(words_supported(n_max, n_win, tab_cap),
             f"n_max {n_max} / n_win {n_win} / tab_cap {tab_cap} beyond hsg_eval_words_supported (1..1024 rows, windows "
             "of 1..8 words, a power of two of 64..8192 slots)")
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
    check(load().hsg_eval_select_words(n, B, ptr(logits), ptr(labels), ptr(doc_off), m, n_max, n_win, ptr(wp), ptr(wi),
                                       tab_cap, ptr(sel), sel_ld, ptr(nsel), ptr(doc_counts), ptr(totals),
                                       stream_of(logits)), "hsg_eval_select_words")
    return sel, nsel, doc_counts


# dataset -> {example index: (ptr, ids) of the whole article}.  train.py's run_eval makes a new
# SLTester per epoch, so the cache lives here, keyed weakly by the dataset, not on the tester.
_WORD_CACHE = weakref.WeakKeyDictionary()


def _cut(entry, n_rows):
    """A whole article's (ptr, ids) for ``n_rows`` sentence nodes."""
    p, ids = entry
    L = len(p) - 1
    if n_rows == L:
        return entry
    if n_rows < L:
        return p[:n_rows + 1], ids[:p[n_rows]]
    return np.concatenate([p, np.full(n_rows - L, p[-1], np.int32)]), ids


def words_for(dataset, index, sents, n_rows):
    """:func:`word_ids` of example ``index`` of ``dataset`` for ``n_rows`` sentence nodes,
    made once per example: the cache holds the whole article and is cut on use.  A dataset
    that cannot be referenced weakly is not cached."""
    try:
        per = _WORD_CACHE.setdefault(dataset, {})
    except TypeError:
        return word_ids(sents, n_rows)
    entry = per.get(index)
    if entry is None:
        entry = per[index] = word_ids(sents)
    return _cut(entry, int(n_rows))


def clear_word_cache():
    """Drop every cached word-id list (after a dataset's texts were changed in place)."""
    _WORD_CACHE.clear()
