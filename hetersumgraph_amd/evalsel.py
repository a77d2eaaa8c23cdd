"""Evaluation-time sentence selection on the native kernel (C ABI: hsg_eval_select,
include/hsg_eval.h, csrc/hsg_eval.hip: the one file of both selection kernels).

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

The last part makes those word ids on the device from the sentences' UTF-8 bytes
(``hsg_eval_text_words``, include/hsg_eval_text.h): :func:`pack_text` and :func:`text_words`.
The host encodes and concatenates; it neither splits nor interns.
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


def _batch(logits, labels, doc_off, m, n_max, totals, sel_ld, out):
    """What :func:`select` and :func:`select_words` share: the checks of the batch's tensors,
    the ``sel_ld`` rule and the outputs, allocated unless given.  Returns (logits, n, B, m,
    n_max, sel_ld, out) with ``logits`` contiguous and the integers as ``int``."""
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
    need = n_max if m == 0 else min(m, n_max)
    sel_ld = need if sel_ld is None else int(sel_ld)
    _require(sel_ld >= need, f"sel_ld {sel_ld} below {need}")
    if out is None:
        out = (torch.empty(B, sel_ld, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, 4, dtype=torch.int32, device=dev))
    for name, t, shape in zip(("sel", "nsel", "doc_counts"), out, ((B, sel_ld), (B,), (B, 4))):
        _require(t.device == dev and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape,
                 f"{name} must be contiguous int32 {shape} on the logits' device")
    return logits.contiguous(), n, B, m, n_max, sel_ld, out


def supported(n_max, gram_max=0):
    return bool(load().hsg_eval_select_supported(int(n_max), int(gram_max)))


def select(logits, labels, doc_off, m, n_max, totals, grams=None, sel_ld=None, out=None):
    """``hsg_eval_select`` on device tensors: returns (sel int32 [B, sel_ld], nsel int32 [B],
    doc_counts int32 [B, 4]) and adds the batch's counters into ``totals`` (int64 [4], on the
    device, accumulated).  ``grams``: a device :class:`GramPack` for n-gram blocking, or
    None.  ``out``: optional (sel, nsel, doc_counts) to write into.  Nothing here waits for
    the device."""
    logits, n, B, m, n_max, sel_ld, (sel, nsel, doc_counts) = _batch(logits, labels, doc_off, m, n_max, totals, sel_ld, out)
    dev, gram_max = logits.device, 0
    gp = gi = gc = None
    if grams is not None:
        _require(grams.buf.device == dev and grams.buf.dtype == torch.int32 and grams.buf.is_contiguous(),
                 "the gram pack must be int32 on the logits' device")
        _require(grams.n == n and grams.B == B, "the gram pack is of another batch")
        gp, gi, gc = grams.views()
        gram_max = int(grams.gram_max)
    _require(supported(n_max, gram_max),
             f"n_max {n_max} / gram_max {gram_max} beyond hsg_eval_select_supported (1..1024 rows, 0..262144 n-grams)")
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
        _require(self.lens is not None, "a word pack made on the device has no word counts on the host: pass tab_cap")
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
    logits, n, B, m, n_max, sel_ld, (sel, nsel, doc_counts) = _batch(logits, labels, doc_off, m, n_max, totals, sel_ld, out)
    dev, n_win = logits.device, int(n_win)
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


# ---- word ids from the sentences' bytes (C ABI: hsg_eval_text_words, include/hsg_eval_text.h) --
# Equal words are equal UTF-8 byte strings and the selection only compares ids with each other,
# so the device can split at str.split()'s whitespace and intern by itself.  The host's part is
# one encode per sentence and one join.

TAB_CAP_MAX = 8192                                         # hsg_eval_words_supported's largest table


class TextPack:
    """One batch's article bytes in ONE uint8 buffer: [byte_ptr (n + 1) int32 | the rows' bytes].
    ``lens`` (bytes per row) and ``counts`` (rows per document) stay on the host for
    :meth:`tab_cap`."""

    def __init__(self, buf, n, B, nbytes, lens, counts):
        self.buf, self.n, self.B, self.nbytes, self.lens, self.counts = buf, n, B, nbytes, lens, counts

    def views(self, buf=None):
        """(byte_ptr int32 [n + 1], text uint8 [nbytes]) as views of ``buf`` (default: this pack's)."""
        buf = self.buf if buf is None else buf
        head = 4 * (self.n + 1)
        return buf[:head].view(torch.int32), buf[head:]

    def to(self, device):
        """The device copy (one non-blocking copy when the host buffer is pinned)."""
        return TextPack(self.buf.to(device, non_blocking=True), self.n, self.B, self.nbytes, self.lens, self.counts)

    def word_bound(self):
        """Per row, the most words its bytes can hold: ceil(L / 2)."""
        return (self.lens + 1) // 2

    def tab_cap(self, n_win, m):
        """Slots of the device's seen set for this batch: :meth:`WordPack.tab_cap`'s rule on the
        per-row bound ceil(L / 2) instead of the true word counts (nobody has counted the
        words), clamped to the kernel's largest table.  A document whose chosen sentences
        really store more windows than that is refused by the kernel, as documented there."""
        cap = WordPack(None, self.n, self.B, 0, self.word_bound(), self.counts).tab_cap(n_win, m)
        return min(cap, TAB_CAP_MAX)


def pack_text(list_of_sents, counts, pin=None):
    """:class:`TextPack` of a batch: ``list_of_sents[d]`` are document d's article sentences,
    ``counts[d]`` its number of sentence nodes.  Only the first ``counts[d]`` sentences are
    taken and rows beyond the article are empty (:func:`word_ids`' rule).  A sentence is
    encoded with ``encode("utf-8", "surrogatepass")``, under which every ``str`` has bytes and
    equal bytes <=> equal ``str``.  The buffer is pinned when a GPU is present (``pin``)."""
    counts = [int(c) for c in counts]
    B, n = len(counts), sum(counts)
    _require(len(list_of_sents) == B, "texts and sentence counts are of different batches")
    lens = np.zeros(n, np.int64)
    encs, row = [], 0
    for sents, c in zip(list_of_sents, counts):
        e = [s.encode("utf-8", "surrogatepass") for s in sents[:c]]
        lens[row:row + len(e)] = [len(x) for x in e]
        encs += e
        row += c
    nbytes = int(lens.sum())
    _require(nbytes < 2 ** 31, "more than 2^31 bytes of text in one batch")
    pin = torch.cuda.is_available() if pin is None else pin
    head = 4 * (n + 1)
    buf = torch.empty(head + nbytes, dtype=torch.uint8, pin_memory=pin)
    a = buf.numpy()
    p = a[:head].view(np.int32)
    p[0] = 0
    np.cumsum(lens, out=p[1:])
    a[head:] = np.frombuffer(b"".join(encs), np.uint8)
    return TextPack(buf, n, B, nbytes, lens, counts)


def text_supported(n, B, nbytes):
    return bool(load().hsg_eval_text_supported(int(n), int(B), int(nbytes)))


def text_words(pack, doc_off=None):
    """``hsg_eval_text_words`` on a device :class:`TextPack`: a device :class:`WordPack` (one
    int32 buffer [word_ptr | word_ids], ``lens = None``) for :func:`select_words`, which then
    needs an explicit ``tab_cap`` (:meth:`TextPack.tab_cap`).  ``doc_off``: the batch's int32
    [B + 1] on the pack's device (default: made from the pack's counts).  Nothing here waits
    for the device."""
    _require(isinstance(pack, TextPack) and torch.is_tensor(pack.buf) and pack.buf.is_cuda
             and pack.buf.dtype == torch.uint8 and pack.buf.is_contiguous(),
             "the text pack must be uint8 on a ROCm device")
    dev, n, B, nbytes = pack.buf.device, pack.n, pack.B, pack.nbytes
    _require(pack.buf.numel() == 4 * (n + 1) + nbytes, "the text pack's buffer is of another batch")
    _require(text_supported(n, B, nbytes),
             f"n {n} / B {B} / nbytes {nbytes} beyond hsg_eval_text_supported (0..2^20 rows, 1..2^20 documents, "
             "0..2^30 bytes)")
    if doc_off is None:
        doc_off = torch.tensor(np.concatenate([[0], np.cumsum(pack.counts)]), dtype=torch.int32).to(dev)
    _require(torch.is_tensor(doc_off) and doc_off.device == dev and doc_off.dtype == torch.int32
             and doc_off.is_contiguous() and doc_off.shape == (B + 1,),
             "doc_off must be contiguous int32 [B + 1] on the pack's device")
    lib = load()
    cap = int(lib.hsg_eval_text_word_bound(n, nbytes))
    out = torch.empty(n + 1 + max(cap, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.hsg_eval_text_workspace_bytes(n, B, nbytes)), dtype=torch.uint8, device=dev)
    byte_ptr, text = pack.views()
    check(lib.hsg_eval_text_words(n, B, ptr(text) if nbytes else None, nbytes, ptr(byte_ptr), ptr(doc_off), cap,
                                  ptr(out), ptr(out[n + 1:]), ptr(ws), stream_of(out)), "hsg_eval_text_words")
    return WordPack(out, n, B, cap, None, pack.counts)
