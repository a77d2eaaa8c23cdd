"""Device-resident document store with on-device batch assembly (opt-in by import).

A document's graph columns, its sentence rows and its two hot relations (W2S, S2W) are pure
functions of the example.  :class:`DocumentStore` builds them once, keeps them on the device
in narrow types, and :meth:`DocumentStore.batch` assembles a batch with four launches
(include/hsg_resident.h: the running offsets, the graph columns, one per relation) instead of
``graph_collate_fn`` + ``DGLGraph.to``: no per-column copy, no segmented sort, and -- unless
the batch needs a work list (``relation.attach_work_lists``) -- no device-to-host copy and no
synchronise.

Why the relations of a batch are the concatenation of its documents': ``hsg_rel_build``'s
CSR is the typed edge list in edge-id order stably sorted by destination rank, its CSC that
CSR stably sorted by source rank, and documents are contiguous in node and edge order -- so
inside a batch every document's slice holds the document's own relation plus five running
offsets (node, edge, source rank, destination rank, typed edge).  tests/resident_ref.py
restates the assembly in numpy and pins it against ``graph.batch`` and the relation oracle.

More of what the model and the evaluation build from a batch is a function of the picked
documents too, so the store hands it over with the batch, as *views*: :class:`ModelView`,
:class:`DocView`, :class:`EvalView`.  Each is one class holding all the store knows of it: what
it validates and keeps per document at build (a document that cannot carry a view makes the
store decline that view; nothing raises), its device columns, the running offsets it adds to a
batch's one pinned copy (:func:`pack_parts`), and its one launch per batch with what that
attaches to the graph.  ``DocumentStore._build`` and ``batch`` loop over ``store.views``;
``model_view=False`` / ``doc_view=False`` / ``eval_view=False`` is the batch without that view.

There is no fallback: a CPU device, a pick outside the store or a batch beyond
``hsg_res_supported`` raises.  Changing a dataset after its store was built is the caller's
business (the store does not look at the dataset again).
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .evalsel import WordPack
from .graph import BatchedDGLGraph, Frame
from .relation import HOT_KINDS, KINDS, Relation, attach_work_lists, build_relation
from .relation import PIECE_MIN, _work_list, piece_params, work_list_capacity

NODE, EDGE, SENT, NFAM = _lib.HSG_RES_NODE, _lib.HSG_RES_EDGE, _lib.HSG_RES_SENT, _lib.HSG_RES_NFAM
SRC, DST, TYP = _lib.HSG_RES_SRC, _lib.HSG_RES_DST, _lib.HSG_RES_TYP
I32_MAX = 2 ** 31 - 1
VIEW_KEYS = (("nodes", "unit", 0.0), ("nodes", "dtype", 1.0), "sent_counts", "tfidf_index", "sent_doc_off")
VIEW_COLUMNS = ("unit", "dtype", "tffrac", "words", "id", "label", "position")
REL_ARRAYS = ("indptr", "src", "tf", "eid", "phantom", "cindptr", "cdst", "cperm", "src_nodes", "dst_nodes")


def _narrow(a, dtype, what, doc):
    """``a`` as ``dtype`` when every value survives the round trip; raises otherwise."""
    a = np.asarray(a)
    b = a.astype(dtype)
    if not np.array_equal(b.astype(a.dtype), a):
        raise ValueError(f"document {doc}: '{what}' holds a value that does not fit {np.dtype(dtype).name}")
    return b


def _pieces(piece_min, piece_mult):
    """The two given, or ``relation.piece_params()``'s in place of a None."""
    if piece_min is None or piece_mult is None:
        pmin, mult = piece_params()
        return pmin if piece_min is None else piece_min, mult if piece_mult is None else piece_mult
    return piece_min, piece_mult


def needs_work_list(n, n_typed, longest, piece_min=None, piece_mult=None):
    """``hsg_rel_work``'s rule on the host: does a CSR / CSC of ``n`` segments over ``n_typed``
    edges, the longest of ``longest`` edges, get a work list?  A segment is split when it is
    longer than ``P = max(PIECE_MIN, PIECE_MULT * ceil(n_typed / n))``."""
    pmin, mult = _pieces(piece_min, piece_mult)
    if n <= 0 or pmin <= 0:
        return False
    return longest > max(pmin, mult * (-(-n_typed // n)))


def batch_order(n_sent):
    """``graph_collate_fn``'s rule made total: descending sentence count, ties in the order
    given (positions into ``n_sent``)."""
    return np.argsort(-np.asarray(n_sent, np.int64), kind="stable")


def doc_counts(doc):
    """Host counts of one ``synth.DocArrays``: ``[NFAM]`` family counts and, per kind, the
    longest CSR (by destination) and CSC (by source) segment of its typed edges."""
    unit, src, dst = np.asarray(doc.unit), np.asarray(doc.src), np.asarray(doc.dst)
    cnt = np.zeros(NFAM, np.int64)
    cnt[NODE], cnt[EDGE], cnt[SENT] = doc.n_nodes, len(src), len(doc.sent_nodes)
    longest = np.zeros((2, 2), np.int64)
    for q, kind in enumerate(HOT_KINDS):
        su, du = KINDS[kind]
        typed = (unit[src] == su) & (unit[dst] == du) if len(src) else np.zeros(0, bool)
        cnt[SRC(q)], cnt[DST(q)], cnt[TYP(q)] = (unit == su).sum(), (unit == du).sum(), typed.sum()
        if typed.any():
            longest[q, 0] = np.bincount(dst[typed]).max()
            longest[q, 1] = np.bincount(src[typed]).max()
    return cnt, longest


def long_segments(doc, above=PIECE_MIN):
    """Per hot kind, the lengths of the CSR (by destination) and CSC (by source) segments of one
    ``synth.DocArrays`` that are longer than ``above``: ``[kind][side]`` int64 arrays.  A piece
    length is never below ``PIECE_MIN``, so these are all a work list's size depends on."""
    unit, src, dst = np.asarray(doc.unit), np.asarray(doc.src), np.asarray(doc.dst)
    out = []
    for kind in HOT_KINDS:
        su, du = KINDS[kind]
        typed = (unit[src] == su) & (unit[dst] == du) if len(src) else np.zeros(0, bool)
        sides = []
        for ends in (dst, src):
            deg = np.bincount(ends[typed]) if typed.any() else np.zeros(0, np.int64)
            sides.append(deg[deg > above].astype(np.int64))
        out.append(sides)
    return out


def work_items(n, n_typed, long_lens, piece_min=None, piece_mult=None, kept=PIECE_MIN):
    """``hsg_rel_work``'s item count on the host, the counterpart of :func:`needs_work_list`:
    for a CSR / CSC of ``n`` segments over ``n_typed`` edges whose segments longer than ``kept``
    have the lengths ``long_lens`` (any order), ``n + sum over deg > P of (ceil(deg / P) - 1)``
    with ``P = max(PIECE_MIN, PIECE_MULT * ceil(n_typed / n))`` -- or 0 when no segment exceeds
    ``P`` (no list).  Raises when ``piece_min`` is below ``kept``: shorter segments could then
    be split, and their lengths were not kept."""
    pmin, mult = _pieces(piece_min, piece_mult)
    if n <= 0 or pmin <= 0:
        return 0
    if pmin < kept:
        raise ValueError(f"work_items: piece_min {pmin} is below the kept threshold {kept}")
    P = max(pmin, mult * (-(-n_typed // n)))
    deg = np.asarray(long_lens, np.int64)
    deg = deg[deg > P]
    if not len(deg):
        return 0
    return int(n + (-(-deg // P) - 1).sum())


HDSG_COLUMNS = {  # the doc view's stored columns by family (include/hsg_resident_hdsg.h)
    "pair": ("pair_s", "pair_d", "doc_sent", "sent_doc"),
    "sent": ("sent_super", "doc_super", "sent_ptr", "sent_row", "sup_list"),
    "docn": ("inv_cnt", "doc_ptr", "doc_row"),
    "sup": ("sup_code", "sup_sent", "sup_ptr"),
}
HDSG_DICT = ("pair_s", "pair_d", "super_pos", "sent_super", "doc_super")        # int64: HiGraph._hdsg_layout's
HDSG_HEAD = ("super_src", "doc_ptr", "doc_sent", "sent_ptr", "sent_doc", "sent_row", "doc_row", "sent_super",
             "doc_super", "sup_sent", "sup_ptr", "sup_list")                    # int32: head.HeadLayout's
HDSG_KEYS = ("hdsg_layout", "hdsg_head_layout")


def doc_view_local(doc, no):
    """``(reason, columns)`` of document ``no``: today's host constructions
    (``HiGraph.hdsg_host_layout``, ``head.HeadLayout``) run on the document alone, as the local
    columns of include/hsg_resident_hdsg.h -- or why the document cannot carry the doc view."""
    from .HiGraph import hdsg_host_layout
    from .head import HeadLayout
    unit, nd = np.asarray(doc.unit), np.asarray(doc.ndtype)
    if not (nd == 2).any():
        return f"document {no}: no doc node (ndtype 2)", None
    try:
        h, n_docs = hdsg_host_layout(unit, nd, np.asarray(doc.src, np.int64), np.asarray(doc.dst, np.int64))
    except AssertionError:
        return f"document {no}: a doc node without a sentence pair", None
    except KeyError as e:
        return f"document {no}: sentence node {e.args[0]} has no doc", None
    lay = HeadLayout(h["pair_s"], h["pair_d"], h["n_s"], n_docs, h["super_pos"], h["sent_super"], h["doc_super"],
                     h["inv_cnt"], "cpu")
    if not lay.ok:
        return f"document {no}: its supernodes (unit 1) are not exactly its sentence and doc nodes", None
    i32 = lambda a: np.asarray(a).astype(np.int32)
    cols = dict(pair_s=i32(h["pair_s"]), pair_d=i32(h["pair_d"]), doc_sent=lay.doc_sent.numpy(),
                sent_doc=lay.sent_doc.numpy(), sent_super=i32(h["sent_super"]), doc_super=i32(h["doc_super"]),
                sent_ptr=lay.sent_ptr.numpy()[:-1], sent_row=lay.sent_row.numpy(), sup_list=lay.sup_list.numpy(),
                inv_cnt=h["inv_cnt"], doc_ptr=lay.doc_ptr.numpy()[:-1], doc_row=lay.doc_row.numpy(),
                sup_code=lay.super_src.numpy(), sup_sent=lay.sup_sent.numpy(), sup_ptr=lay.sup_ptr.numpy()[:-1])
    return None, cols


def eval_view_local(entry, n_sent):
    """The local columns of one document's ``eval_words`` entry for its ``n_sent`` sentence rows
    (include/hsg_resident_eval.h) -- ``dict(wend=ptr[1:] int32, wid=ids int32, lens=words per
    row int64)`` -- or, as a ``str``, why the entry cannot carry the eval view.  Accepted: a list
    of exactly one ``(ptr, ids)`` pair of ``evalsel.word_ids``' form: integral 1-D arrays,
    ``len(ptr) == n_sent + 1``, ``ptr[0] == 0``, ``ptr`` non-decreasing, ``ptr[-1] == len(ids)``,
    ids that fit int32."""
    if not isinstance(entry, (list, tuple)):
        return f"its eval_words entry is a {type(entry).__name__}, not a list of one (ptr, ids) pair"
    if len(entry) != 1:
        return f"its eval_words entry has {len(entry)} parts, not one (ptr, ids) pair"
    pair = entry[0]
    if not isinstance(pair, (list, tuple)) or len(pair) != 2:
        return "its eval_words part is not a (ptr, ids) pair"
    ptr_, ids = np.asarray(pair[0]), np.asarray(pair[1])
    if ptr_.ndim != 1 or ids.ndim != 1 or ptr_.dtype.kind not in "iu" or (ids.size and ids.dtype.kind not in "iu"):
        return "its (ptr, ids) are not one-dimensional integer arrays"
    if len(ptr_) != int(n_sent) + 1:
        return f"its word ptr has {len(ptr_)} elements for {int(n_sent)} sentence rows (rows + 1 expected)"
    ptr_ = ptr_.astype(np.int64)
    if ptr_[0] != 0:
        return f"its word ptr begins at {int(ptr_[0])}, not 0"
    lens = np.diff(ptr_)
    if (lens < 0).any():
        return "its word ptr decreases"
    if ptr_[-1] != len(ids):
        return f"its word ptr ends at {int(ptr_[-1])} for {len(ids)} word ids"
    if ids.size and (int(ids.min()) < -I32_MAX - 1 or int(ids.max()) > I32_MAX):
        return "a word id does not fit int32"
    return dict(wend=ptr_[1:].astype(np.int32), wid=ids.astype(np.int32), lens=lens)


def seen_columns(lens):
    """``(lens_desc, doc_of_row, rank)`` of :func:`seen_need` from every document's words per
    row (a list of int arrays, one per document)."""
    n_rows = np.asarray([len(a) for a in lens], np.int64)
    lens_desc = np.concatenate([-np.sort(-np.asarray(a, np.int64)) for a in lens] or [np.zeros(0, np.int64)])
    doc_of_row = np.repeat(np.arange(len(lens)), n_rows)
    rank = np.arange(len(doc_of_row)) - np.repeat(np.cumsum(n_rows) - n_rows, n_rows)
    return lens_desc, doc_of_row, rank


def seen_need(lens_desc, doc_of_row, rank, n_docs, n_win, m):
    """Per document, ``evalsel.WordPack.win_need``'s term: the sum of the ``min(m, N_d)`` largest
    per-row window counts ``max(len - n_win, 0)``.  ``lens_desc``: every document's words per row,
    each document's sorted descending (subtracting ``n_win`` keeps that order); ``doc_of_row`` and
    ``rank``: the row's document and its position inside it.  int64 ``[n_docs]``."""
    win = np.maximum(lens_desc - int(n_win), 0) * (rank < int(m))
    return np.bincount(doc_of_row, weights=win, minlength=n_docs).astype(np.int64)


def sentence_layout(words):
    """Host statement of ``cnn._layout`` for one document's token rows [N, L]: (length [N],
    the exclusive prefix of ``length + 1`` [N], the row count, whether a non-zero token follows
    a PAD)."""
    words = np.asarray(words)
    nz = words != 0
    length = nz.sum(1).astype(np.int64)
    inner = bool((nz & (np.arange(words.shape[1])[None, :] >= length[:, None])).any())
    pre = np.zeros(len(length), np.int64)
    np.cumsum(length[:-1] + 1, out=pre[1:])
    return length, pre, int((length + 1).sum()), inner


def view_refusal(doc, no):
    """Why document ``no`` cannot carry the model view (None: it can)."""
    words = np.asarray(doc.words)
    if sentence_layout(words)[3]:
        return f"document {no}: token ids after the first PAD (0) -- padding must be trailing"
    if (words < 0).any():
        return f"document {no}: a negative token id"
    if not np.array_equal(np.nonzero(np.asarray(doc.ndtype) == 1)[0], np.asarray(doc.sent_nodes, np.int64)):
        return f"document {no}: the sentence nodes are not the dtype-1 nodes in ascending order"
    return None


class ModelInputs:
    """The model view of one resident batch (include/hsg_resident_model.h): device tensors
    ``sent_nodes``, ``sent_ids``, ``sent_pos``, ``sent_len``, ``rowoff``, ``doc_off``, ``prev``,
    ``tfidf_index``; host ``rows`` (the CNN's row count), ``bound`` (1 + the sum of the
    documents' distinct non-zero tokens: at least the batch's distinct tokens, PAD included)
    and ``max_token`` (the store's largest token id); ``glen``, the sentences per document."""

    def __init__(self, glen, rows, bound, max_token, **tensors):
        self.glen, self.rows, self.bound, self.max_token = tuple(glen), int(rows), int(bound), int(max_token)
        self.__dict__.update(tensors)
        self._lstm = None

    @property
    def layout(self):
        """What ``cnn._layout`` returns for ``sent_ids``, with the largest token id for the
        range check on the host."""
        from .cnn import BatchLayout
        return BatchLayout(self.sent_len, self.rowoff, self.rows, self.max_token)

    @property
    def doc_layout(self):
        """The ``lstm.DocLayout`` of the batch, from ``doc_off`` and ``prev``."""
        if self._lstm is None:
            from .lstm import DocLayout
            self._lstm = DocLayout.prebuilt(self.glen, self.doc_off, self.prev)
        return self._lstm


class ResidentWordPack(WordPack):
    """The eval view of one resident batch (include/hsg_resident_eval.h): an
    ``evalsel.WordPack`` whose buffer was assembled on the device -- bit-equal to
    ``pack_words(G.eval_words, counts).buf`` -- and whose :meth:`win_need` (so ``tab_cap``) is one
    ``max`` over the store's cached per-document values instead of a sort per document."""

    def __init__(self, buf, n, B, W, counts, store, slots):
        super().__init__(buf, n, B, W, None, counts)
        self._store, self._slots = store, slots

    def to(self, device):
        if _device(device, allow_cpu=True) == self.buf.device:
            return self
        return ResidentWordPack(self.buf.to(device, non_blocking=True), self.n, self.B, self.W, self.counts,
                                self._store, self._slots)

    def win_need(self, n_win, m):
        return int(self._store.seen_need(n_win, m)[self._slots].max(initial=0))


class ResidentBatch(BatchedDGLGraph):
    """A batch assembled by :meth:`DocumentStore.batch`: a ``BatchedDGLGraph`` on the store's
    device whose frames and relations are already there.  The host-side structural views
    (``host_column``, ``_src`` / ``_dst``) come from the store's host copies of the picked
    documents: the node views eagerly, the edge views on first use."""

    def __init__(self):
        self._h_src = self._h_dst = None
        self._origin = None               # (store, slots) until a structural column is written
        self._view = None                 # (ModelInputs, the columns it restates with their versions)
        super().__init__()

    @property
    def model_inputs(self):
        """The batch's :class:`ModelInputs`, or None: no view was assembled, or a column it
        restates was written since (by assignment, or in place: the tensor's version moved)."""
        if self._view is not None:
            nd = self._nframe.cols
            if any(nd.get(k) is not t or t._version != ver for k, t, ver in self._view[1]):
                self._drop_view()
        return None if self._view is None else self._view[0]

    def _set_view(self, view):
        nd = self._nframe.cols
        self._view = (view, [(k, nd[k], nd[k]._version) for k in ("words", "position")])

    def _drop_view(self):
        self._view = None
        for key in VIEW_KEYS + HDSG_KEYS:                 # the doc view goes with the rest of the view
            self._rel_cache.pop((key, str(self.device)), None)

    def _edges(self):
        if self._h_src is None and self._origin is not None:
            store, slots = self._origin
            self._h_src, self._h_dst = store._host_edge_lists(slots)

    @property
    def _src(self):
        self._edges()
        return self._h_src

    @_src.setter
    def _src(self, v):
        self._h_src = v

    @property
    def _dst(self):
        self._edges()
        return self._h_dst

    @_dst.setter
    def _dst(self, v):
        self._h_dst = v

    def number_of_edges(self):
        if self._origin is not None and not self._pending:
            return int(sum(self.batch_num_edges))
        return super().number_of_edges()

    num_edges = number_of_edges

    def _src_t(self):
        if self._dev_src is None:
            return super()._src_t()
        return self._dev_src

    def host_column(self, key):
        if self._origin is not None and key in ("tffrac", "edtype") and key not in self._host_cols:
            store, slots = self._origin
            self._host_cols.update(store._host_edge_columns(slots))
        return super().host_column(key)

    def _detach(self):
        """A structural write: the store's host copies no longer describe this graph."""
        self._drop_view()
        if self._origin is not None:
            self._edges()
            self._origin = None

    def _mutated(self):
        self._detach()
        super()._mutated()

    def _touch_column(self, key, is_node):
        if key in VIEW_COLUMNS:
            self._drop_view()
        if key in ("unit", "dtype", "tffrac"):
            self._detach()
        super()._touch_column(key, is_node)

    def to(self, device, **kwargs):
        device = _device(device, allow_cpu=True)
        if device == self.device:
            return self
        self._detach()
        return super().to(device, **kwargs)

    def __getstate__(self):
        self._detach()
        return super().__getstate__()


def _device(device, allow_cpu=False):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda" and not allow_cpu:
        raise RuntimeError("the resident document store lives on a ROCm device (hsg_res_*); no CPU fallback")
    return device


def _starts(counts):
    """The exclusive prefix sums of ``counts`` and their total: int64 ``[len(counts) + 1]``."""
    out = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def pack_parts(parts):
    """What one pinned copy of a batch carries: ``parts`` (the pick list, then every active
    view's running offsets) end to end as one int32 array, and the slice of each part in it."""
    cuts, at = [], 0
    for a in parts:
        cuts.append(slice(at, at + len(a)))
        at += len(a)
    return np.concatenate(parts).astype(np.int32), cuts


# ---------------------------------------------------------------------- views
# What a store knows about one view of its batches, in one common shape: ``ok`` / ``reason``;
# ``add(doc, no)`` per document at build (it declines and never raises; a view that declined is
# not called again unless ``always``); ``finish(device)`` concatenates, uploads (``cols``) and fills ``cstruct``;
# ``offsets(lib, slots, tot)`` gives the view's running sums over the sorted pick ([B + 1] int64
# each, they ride in the batch's pinned copy) after its ``*_supported`` check; ``assemble(b, host,
# dev)`` allocates the outputs, launches and attaches them to ``b.G``, ``host`` / ``dev`` being
# those offsets as given and as they arrived on the device, ``b`` the batch's store, library,
# slots, totals, sentence counts, allocator and launch operands.  ``needs``: the view this one is only attached with.
class _View:
    flag = needs = None               # ``flag``: batch()'s keyword, and the store's attribute
    always = False                    # True: built and kept for a store that declined it too
    checked = 1                       # the order in which batch() runs the ``*_supported`` checks

    def __init__(self, *parts):
        self.ok, self.reason = True, None
        self.cols, self.cstruct = {}, None
        self._parts = {k: [] for k in parts}          # per document, until finish()

    def decline(self, reason):
        self.ok, self.reason = False, reason

    def keep(self, arrays):
        for k, a in arrays.items():
            self._parts[k].append(a)

    def upload(self, arrays, device):
        self.cols = {k: torch.from_numpy(np.ascontiguousarray(a)).to(device) for k, a in arrays.items()}
        self._parts = None

    def tensors(self):
        return list(self.cols.values())


class ModelView(_View):
    """include/hsg_resident_model.h: the model's index structures (``G.model_inputs``, a
    :class:`ModelInputs`, and the entries the model caches on the graph), so a forward starts
    without the host-built indices and the host waits it otherwise begins with.  Host:
    ``rows_of`` (CNN rows, ``sum(length + 1)``) and ``distinct`` (distinct non-zero tokens) per
    document, ``max_token`` of the store -- kept, with the columns, for a store that declined the
    view too, as they always were (``store.distinct``, ``store.nbytes``)."""
    flag, always = "model_view", True

    def __init__(self):
        super().__init__("tok_len", "tok_row", "rows", "distinct")
        self.max_token = 0

    def add(self, doc, no):
        reason = view_refusal(doc, no) if self.ok else None
        if reason is not None:
            self.decline(reason)
        # per sentence its length and row offset (cnn._layout's rule)
        words = np.asarray(doc.words)
        length, pre, n_rows, _ = sentence_layout(words)
        self.keep(dict(tok_len=length.astype(np.int32), tok_row=pre.astype(np.int32), rows=n_rows,
                       distinct=int(np.count_nonzero(np.unique(words)))))
        self.max_token = max(self.max_token, int(words.max()) if words.size else 0)

    def finish(self, device):
        p = self._parts
        self.rows_of, self.distinct = np.asarray(p["rows"], np.int64), np.asarray(p["distinct"], np.int64)
        self.upload({k: np.concatenate(p[k]) for k in ("tok_len", "tok_row")}, device)

    def offsets(self, lib, slots, tot):
        rowbase = _starts(self.rows_of[slots])
        B, n_s, rows = len(slots), int(tot[SENT]), int(rowbase[-1])
        if not lib.hsg_res_model_supported(B, n_s, int(tot[EDGE]), rows):
            raise RuntimeError(f"batch of {B} documents, {n_s} sentences, {rows} token rows: "
                               "beyond hsg_res_model_supported")
        return [rowbase]

    def assemble(self, b, host, dev):
        G, new, p, i64, i32 = b.G, b.new, _lib.ptr, torch.int64, torch.int32
        B, n_s, E, L = len(b.slots), int(b.tot[SENT]), int(b.tot[EDGE]), b.store.sent_len
        t = dict(sent_nodes=new(n_s, i64), sent_ids=new((n_s, L), i64), sent_pos=new(n_s, i64),
                 sent_len=new(n_s, i64), rowoff=new(n_s + 1, i32), doc_off=new(B + 1, i32),
                 prev=new((n_s, 2), i64), tfidf_index=new(E, i64))
        _lib.check(b.lib.hsg_res_model(b.cs, p(self.cols["tok_len"]), p(self.cols["tok_row"]), B, p(b.pick),
                                       p(b.offs), p(dev[0]), n_s, E, *[p(v) for v in t.values()], b.st),
                   "hsg_res_model")
        glen = b.glen
        G._set_view(ModelInputs(glen, host[0][B], 1 + int(self.distinct[b.slots].sum()), self.max_token, **t))
        # under the keys HiGraph._cached uses; the word nodes are the W2S relation's sources
        words = G._rel_cache[("rel", "W2S", str(G.device))].dev["src_nodes"]
        for key, val in zip(VIEW_KEYS, (words, t["sent_nodes"], glen, t["tfidf_index"], t["doc_off"])):
            G._rel_cache[(key, str(G.device))] = val


class DocView(_View):
    """include/hsg_resident_hdsg.h: the entries ``HiGraph._hdsg_layout`` and ``_hdsg_head_layout``
    cache on the graph, from each document's local form of them; only attached with the model
    view.  Host: ``docn`` (doc nodes) and ``pairs`` (sentence -> doc pairs) per document, and the
    lengths of the segments longer than ``PIECE_MIN`` (``long_lens`` ``[kind][side]``, every
    document's end to end, beginning at ``long_starts``), from which the view sizes a batch's
    work lists on the host instead of reading their counts back."""
    flag = "doc_view"

    def __init__(self, model):
        super().__init__(*[k for fam in HDSG_COLUMNS.values() for k in fam])
        self.needs = model
        self._long = [[[], []] for _ in HOT_KINDS]

    def add(self, doc, no):
        reason, local = doc_view_local(doc, no)
        if reason is not None:
            return self.decline(reason)
        self.keep(local)
        for q, sides in enumerate(long_segments(doc)):
            for side, lens in enumerate(sides):
                self._long[q][side].append(lens)

    def finish(self, device):
        p = self._parts
        self.docn = np.asarray([len(a) for a in p["inv_cnt"]], np.int64)
        self.pairs = np.asarray([len(a) for a in p["pair_s"]], np.int64)
        self.long_lens = [[np.concatenate(v) for v in sides] for sides in self._long]
        self.long_starts = [[_starts([len(a) for a in v]) for v in sides] for sides in self._long]
        self._long = None
        self.upload(dict({k: np.concatenate(v) for k, v in p.items()}, dstart=_starts(self.docn),
                         pstart=_starts(self.pairs)), device)
        self.cstruct = _lib.HsgResHdsgCols(**{k: _lib.ptr(v) for k, v in self.cols.items()})

    def offsets(self, lib, slots, tot):
        docbase, pairbase = _starts(self.docn[slots]), _starts(self.pairs[slots])
        B, n_dn, n_pr = len(slots), int(docbase[-1]), int(pairbase[-1])
        if not lib.hsg_res_hdsg_supported(B, int(tot[SENT]), n_dn, n_pr, int(tot[DST(0)])):
            raise RuntimeError(f"batch of {B} documents, {n_dn} doc nodes, {n_pr} sentence-doc pairs: "
                               "beyond hsg_res_hdsg_supported")
        return [docbase, pairbase]

    def work_lists(self, b, q, d, ns, ndst, nt, pieces):
        """Relation ``q``'s work lists onto its arrays ``d`` with each side's item count from the
        kept segment lengths: the unchanged ``hsg_rel_work`` into today's buffer, sliced by that
        count; nothing is read back.  False (nothing done) when shorter segments could split."""
        if pieces[0] < PIECE_MIN:
            return False
        for key, side, n, ptr_key in (("dwork", 0, ndst, "indptr"), ("swork", 1, ns, "cindptr")):
            a, st = self.long_lens[q][side], self.long_starts[q][side]
            items = work_items(n, nt, np.concatenate([a[st[s]:st[s + 1]] for s in b.slots]), *pieces)
            cap = work_list_capacity(n, nt, pieces[0])
            if items > 0 and not n <= items <= cap:
                raise AssertionError(f"work list of {items} items for {n} segments: outside [n, {cap}]")
            if items > 0:
                d[key] = _work_list(b.lib, n, d[ptr_key], nt, b.st, read_back=False, pieces=pieces)[0][:5 * items]
        return True

    def assemble(self, b, host, dev):
        from .head import HeadLayout
        G, new, p, B = b.G, b.new, _lib.ptr, len(b.slots)
        n_s, n_dn, n_pr, n_su = int(b.tot[SENT]), int(host[0][B]), int(host[1][B]), int(b.tot[DST(0)])
        sizes = dict(pair_s=n_pr, pair_d=n_pr, super_pos=n_su, sent_super=n_s, doc_super=n_s, super_src=n_su,
                     doc_ptr=n_dn + 1, doc_sent=n_pr, sent_ptr=n_s + 1, sent_doc=n_pr, sent_row=n_s,
                     doc_row=n_dn, sup_sent=n_su, sup_ptr=n_su + 1, sup_list=n_s)
        lay = {k: new(sizes[k], torch.int64) for k in HDSG_DICT}
        inv_cnt = new(n_dn, torch.float32)
        lists = {k: new(sizes[k], torch.int32) for k in HDSG_HEAD}
        _lib.check(b.lib.hsg_res_hdsg(b.cs, ctypes.byref(self.cstruct), B, p(b.pick), p(b.offs), p(dev[0]),
                                      p(dev[1]), n_s, n_dn, n_pr, n_su, *[p(v) for v in lay.values()],
                                      p(inv_cnt), *[p(v) for v in lists.values()], b.st), "hsg_res_hdsg")
        # under the keys HiGraph._hdsg_layout / _hdsg_head_layout use
        G._rel_cache[(HDSG_KEYS[0], str(G.device))] = dict(lay, inv_cnt=inv_cnt, n_docs=n_dn)
        G._rel_cache[(HDSG_KEYS[1], str(G.device))] = HeadLayout.prebuilt(n_s, n_dn, n_su, inv_cnt, **lists)


class EvalView(_View):
    """include/hsg_resident_eval.h: the evaluation step's blocking operand (``G.eval_pack``, a
    :class:`ResidentWordPack` bit-equal to ``evalsel.pack_words(G.eval_words, counts)``) from each
    document's local ``(ptr, ids)``; a store built without ``eval_words``, or with an entry of
    another form than one ``word_ids`` pair, declines it.  Independent of the other views.  Host:
    ``words_of`` (words per document) and what sizes the seen set (:meth:`seen_need`)."""
    flag, checked = "eval_view", 0

    def __init__(self, eval_words):
        super().__init__("wend", "wid", "lens")
        self._words, self._need = eval_words, {}
        if eval_words is None:
            self.decline("the store was built without eval_words")

    def add(self, doc, no):
        ew = "it has no eval_words entry"
        if no < len(self._words):
            ew = eval_view_local(self._words[no], len(doc.sent_nodes))
        if isinstance(ew, str):
            return self.decline(f"document {no}: {ew}")
        self.keep(ew)

    def finish(self, device):
        p = self._parts
        self.words_of = np.asarray([len(a) for a in p["wid"]], np.int64)
        # every document's words per row sorted descending, each row's document and its position
        # inside it (seen_need)
        self._seen = seen_columns(p["lens"])
        self.upload(dict(wstart=_starts(self.words_of), wend=np.concatenate(p["wend"]), wid=np.concatenate(p["wid"])),
                    device)
        self.cstruct = _lib.HsgResEvalCols(**{k: _lib.ptr(v) if v.numel() else None for k, v in self.cols.items()})

    def seen_need(self, n_win, m):
        """Per document of the store, :func:`seen_need` for windows of ``n_win`` words and ``m``
        chosen sentences: int64 ``[n_docs]``, computed once per pair and kept."""
        key = (int(n_win), int(m))
        if key not in self._need:
            if not self.ok:
                raise RuntimeError("the store declined the eval view: " + self.reason)
            self._need[key] = seen_need(*self._seen, len(self.words_of), *key)
        return self._need[key]

    def offsets(self, lib, slots, tot):
        wordbase = _starts(self.words_of[slots])
        B, n_s, n_w = len(slots), int(tot[SENT]), int(wordbase[-1])
        if not lib.hsg_res_eval_supported(B, n_s, n_w):
            raise RuntimeError(f"batch of {B} documents, {n_s} sentences, {n_w} words: beyond "
                               "hsg_res_eval_supported")
        return [wordbase]

    def assemble(self, b, host, dev):
        p, B, n_s, n_w = _lib.ptr, len(b.slots), int(b.tot[SENT]), int(host[0][-1])
        pack = b.new(n_s + 1 + max(n_w, 1), torch.int32)
        _lib.check(b.lib.hsg_res_eval(b.cs, ctypes.byref(self.cstruct), B, p(b.pick), p(b.offs), p(dev[0]), n_s,
                                      n_w, p(pack), b.st), "hsg_res_eval")
        b.G.eval_pack = ResidentWordPack(pack, n_s, B, n_w, list(b.glen), b.store, b.slots)


STORE_COLUMNS = ("unit", "ndtype", "id", "sent_rank", "words", "label", "src", "dst", "tffrac", "edtype")


class DocumentStore:
    """Every document of a dataset, on the device (see the module docstring)."""

    MODEL_VIEW = True                 # batch()'s default for ``model_view`` (measured: DESIGN.md §6)
    DOC_VIEW = True                   # batch()'s default for ``doc_view`` (measured: DESIGN.md §6)
    EVAL_VIEW = True                  # batch()'s default for ``eval_view`` (measured: DESIGN.md §6)

    # ------------------------------------------------------------------ build
    def __init__(self, device):
        self.device = _device(device)
        self._docs = 0

    @classmethod
    def from_doc_arrays(cls, docs, device, chunk=256, indices=None, eval_words=None):
        """``docs``: a list of ``synth.DocArrays``; ``indices``: the dataset index of each
        (default: its position); ``eval_words``: per document, what ``G.eval_words`` of its
        one-member batch holds (``ExampleSet(eval_words=True)``)."""
        docs = list(docs)
        eval_words = None if eval_words is None else list(eval_words)
        return cls._build([docs[i:i + chunk] for i in range(0, len(docs), max(1, int(chunk)))], device, indices,
                          eval_words)

    @classmethod
    def from_dataset(cls, dataset, device, indices=None, chunk=256):
        """``dataset``: an ``ExampleSet`` / ``MultiExampleSet``; the documents come from
        ``dataset.graph_arrays`` in chunks of ``chunk``."""
        indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
        words = [] if getattr(dataset, "eval_words", False) else None

        def chunks():
            for i in range(0, len(indices), max(1, int(chunk))):
                idx = indices[i:i + chunk]
                if words is None:
                    yield dataset.graph_arrays(idx)
                    continue
                from .evalsel import word_ids
                items = [dataset.get_example(j) for j in idx]
                for it in items:
                    rows = min(len(it.original_article_sents), dataset.doc_max_timesteps)
                    words.append([word_ids(it.original_article_sents, rows)])
                yield dataset.graph_arrays(idx, items)
        return cls._build(chunks(), device, indices, words)

    @classmethod
    def _build(cls, chunks, device, indices, eval_words):
        self = cls(device)
        model = ModelView()
        self.views = {v.flag: v for v in (model, DocView(model), EvalView(eval_words))}     # in launch order
        self.sent_len = self.label_len = None
        acc = SimpleNamespace(counts=[], longest=[], bases=[], cols={k: [] for k in STORE_COLUMNS},
                              host={k: [] for k in ("unit", "ndtype", "src", "dst", "tffrac", "edtype")},
                              rels=[{k: [] for k in REL_ARRAYS} for _ in HOT_KINDS])
        for docs in chunks:
            if not docs:
                continue
            base = np.zeros(NFAM, np.int64)
            part = {k: [] for k in STORE_COLUMNS}
            for doc in docs:
                no = len(acc.counts)
                cnt, lng = self._add_document(doc, no, base, acc.host, part)
                for v in self.views.values():
                    if v.ok or v.always:        # a view that declined does no more work
                        v.add(doc, no)
                acc.counts.append(cnt)
                acc.longest.append(lng)
                acc.bases.append(base.copy())
                base += cnt
            self._upload_chunk(part, base, acc)
        self._close(acc, indices, eval_words)
        return self

    def _add_document(self, doc, no, base, host, part):
        """The store's own step for document ``no``, ``base`` of its families into its chunk:
        validation, narrowing, the host copies and the chunk's columns.  Its counts and longest
        segments (:func:`doc_counts`)."""
        cnt, lng = doc_counts(doc)
        n, N = int(cnt[NODE]), int(cnt[SENT])
        words, label = np.asarray(doc.words), np.asarray(doc.label)
        if words.ndim != 2 or label.ndim != 2 or len(words) != N or len(label) != N:
            raise ValueError(f"document {no}: 'words' / 'label' are not [sentences, width]")
        if self.sent_len is None:
            self.sent_len, self.label_len = int(words.shape[1]), int(label.shape[1])
        if (words.shape[1], label.shape[1]) != (self.sent_len, self.label_len):
            raise ValueError(f"document {no}: sentence rows of another width than the store's")
        if not np.array_equal(np.asarray(doc.position).reshape(-1), np.arange(1, N + 1)):
            raise ValueError(f"document {no}: 'position' is not 1..N (the store does not keep it)")
        sn = np.asarray(doc.sent_nodes, np.int64)
        if len(np.unique(sn)) != N or (N and (sn.min() < 0 or sn.max() >= n)):
            raise ValueError(f"document {no}: sentence nodes repeat or lie outside the document")
        if cnt[EDGE] and (min(doc.src.min(), doc.dst.min()) < 0 or max(doc.src.max(), doc.dst.max()) >= n):
            raise ValueError(f"document {no}: an edge references a node outside the document")
        if base[NODE] + n > I32_MAX or base[EDGE] + cnt[EDGE] > I32_MAX:
            raise ValueError("a build chunk beyond 2^31 - 1 nodes or edges: use a smaller chunk")
        rank = np.full(n, -1, np.int32)
        rank[sn] = np.arange(N, dtype=np.int32)
        u8 = {k: _narrow(getattr(doc, k), np.uint8, k, no) for k in ("unit", "ndtype", "tffrac", "edtype")}
        src, dst = _narrow(doc.src, np.int32, "src", no), _narrow(doc.dst, np.int32, "dst", no)
        for k in ("unit", "ndtype", "tffrac", "edtype"):
            host[k].append(u8[k])
            part[k].append(u8[k])
        host["src"].append(src)
        host["dst"].append(dst)
        part["src"].append(src + np.int32(base[NODE]))
        part["dst"].append(dst + np.int32(base[NODE]))
        part["id"].append(_narrow(doc.wid, np.int32, "id", no))
        part["sent_rank"].append(rank)
        part["words"].append(_narrow(words, np.int32, "words", no).reshape(-1))
        part["label"].append(_narrow(label, np.uint8, "label", no).reshape(-1))
        return cnt, lng

    def _upload_chunk(self, part, base, acc):
        """One build chunk: its columns to the device, and its relations by today's builder
        (chunk-relative values are kept as they are).  ``base``: the chunk's family totals."""
        cat = {k: torch.from_numpy(np.concatenate(v)).to(self.device) for k, v in part.items()}
        for k, v in cat.items():
            acc.cols[k].append(v)
        for q, kind in enumerate(HOT_KINDS):
            rel = build_relation(kind, cat["src"], cat["dst"], cat["unit"], cat["tffrac"], cat["edtype"])
            if (rel.n_src, rel.n_dst, rel.n_typed) != (base[SRC(q)], base[DST(q)], base[TYP(q)]):
                raise RuntimeError(f"{kind}: hsg_rel_build disagrees with the host counts of the chunk")
            d = rel.dev
            for k in REL_ARRAYS:
                a = d[k][:rel.n_dst] if k == "indptr" else d[k][:rel.n_src] if k == "cindptr" else d[k]
                acc.rels[q][k].append(a.to(torch.uint8 if k == "tf" else torch.int32))

    def _close(self, acc, indices, eval_words):
        """The closing step of a build: the host tables, the views, the device struct."""
        if not acc.counts:
            raise ValueError("an empty document store")
        dev = self.device
        self._docs = len(acc.counts)
        self.counts = np.stack(acc.counts)                                # [n_docs, NFAM]
        self.longest = np.stack(acc.longest)                              # [n_docs, kind, CSR / CSC]
        self.starts = np.zeros((NFAM, self._docs + 1), np.int64)
        self.starts[:, 1:] = np.cumsum(self.counts, 0).T
        self.bases = np.ascontiguousarray(np.stack(acc.bases).T)          # [NFAM, n_docs]
        self.indices = list(range(self._docs)) if indices is None else [int(i) for i in indices]
        if len(self.indices) != self._docs or len(set(self.indices)) != self._docs:
            raise ValueError("indices: one distinct dataset index per document")
        self._slot_of = {ix: s for s, ix in enumerate(self.indices)}
        self.eval_words = None if eval_words is None else list(eval_words)
        self._host = {k: np.concatenate(v) for k, v in acc.host.items()}
        self._cols = {k: torch.cat(v) for k, v in acc.cols.items()}
        self._rels = [{k: torch.cat(v) for k, v in r.items()} for r in acc.rels]
        for v in self.views.values():
            if v.ok and v.needs is not None and not v.needs.ok:
                v.decline(f"the store declined the {v.needs.flag.replace('_', ' ')}: {v.needs.reason}")
            if v.ok or v.always:
                v.finish(dev)
            setattr(self, v.flag, v.ok)                 # store.model_view, store.model_view_reason, ...
            setattr(self, v.flag + "_reason", v.reason)
        self._starts_d = torch.from_numpy(self.starts).to(dev)
        self._bases_d = torch.from_numpy(self.bases).to(dev)
        p = _lib.ptr
        self._cstruct = _lib.HsgResStore(
            self._docs, p(self._starts_d), p(self._bases_d), self.sent_len, self.label_len,
            *[p(self._cols[k]) for k in STORE_COLUMNS],
            (_lib.HsgResRel * 2)(*[_lib.HsgResRel(*[p(r[k]) for k in REL_ARRAYS]) for r in self._rels]))
        torch.cuda.synchronize(dev)        # the build's host arrays may go once the uploads are done

    def __len__(self):
        return self._docs

    distinct = property(lambda self: self.views["model_view"].distinct)
    words_of = property(lambda self: self.views["eval_view"].words_of)

    def seen_need(self, n_win, m):
        """:meth:`EvalView.seen_need`."""
        return self.views["eval_view"].seen_need(n_win, m)

    def _tensors(self):
        return list(self._cols.values()) + [t for v in self.views.values() for t in v.tensors()] + \
            [t for r in self._rels for t in r.values()] + [self._starts_d, self._bases_d]

    @property
    def nbytes(self):
        """Bytes of device memory the store holds."""
        return int(sum(t.numel() * t.element_size() for t in self._tensors()))

    # ------------------------------------------------------------ host views
    def _host_slices(self, key, fam, slots):
        a, st = self._host[key], self.starts[fam]
        return [a[st[s]:st[s + 1]] for s in slots]

    def _host_node_columns(self, slots):
        f = lambda k: np.concatenate(self._host_slices(k, NODE, slots)).astype(np.float32)
        return {"unit": f("unit"), "ndtype": f("ndtype")}

    def _host_edge_columns(self, slots):
        cat = lambda k: np.concatenate(self._host_slices(k, EDGE, slots))
        return {"tffrac": cat("tffrac").astype(np.int64), "edtype": cat("edtype").astype(np.float32)}

    def _host_edge_lists(self, slots):
        noff = np.concatenate([[0], np.cumsum(self.counts[slots, NODE])])
        out = []
        for k in ("src", "dst"):
            out.append(np.concatenate([a.astype(np.int64) + o
                                       for a, o in zip(self._host_slices(k, EDGE, slots), noff)] or
                                      [np.zeros(0, np.int64)]))
        return tuple(out)

    # ----------------------------------------------------------------- batch
    def slots_of(self, indices):
        try:
            return np.asarray([self._slot_of[int(i)] for i in indices], np.int64)
        except KeyError as e:
            raise IndexError(f"document {e.args[0]} is not in the store") from None

    def batch(self, indices, model_view=None, doc_view=None, eval_view=None):
        """``(G, index)`` as ``graph_collate_fn`` gives them for the same documents: sorted by
        sentence count (descending, ties in the order given), ``G`` on the device.

        ``model_view``, ``doc_view``, ``eval_view``: None (the store's default, :attr:`MODEL_VIEW`,
        :attr:`DOC_VIEW`, :attr:`EVAL_VIEW`), True or False -- whether the batch carries that
        view (:class:`ModelView`, :class:`DocView`, :class:`EvalView`), each assembled by one more
        launch.  A view the store declined at build (``store.model_view`` False,
        ``store.model_view_reason``, and so on) is never attached, nor is one without the view
        it needs: the doc view rides on the model view; the evaluation's is independent of both.
        With the doc view the batch's work lists are sized on the host instead of read back.
        False is the batch without the view, bit for bit (read-back included);
        ``G.eval_words`` is attached either way."""
        want, active = dict(model_view=model_view, doc_view=doc_view, eval_view=eval_view), []
        for v in self.views.values():
            on = getattr(self, v.flag.upper()) if want[v.flag] is None else bool(want[v.flag])
            if v.ok and on and (v.needs is None or v.needs in active):
                active.append(v)
        slots = self.slots_of(indices)
        B = len(slots)
        if B < 1:
            raise ValueError("an empty batch")
        slots = slots[batch_order(self.counts[slots, SENT])]
        tot = self.counts[slots].sum(0)
        lib, dev = _lib.load(), self.device
        n, E = int(tot[NODE]), int(tot[EDGE])
        if not lib.hsg_res_supported(B, n, E, int(max(tot[TYP(0)], tot[TYP(1)]))):
            raise RuntimeError(f"batch of {B} documents, {n} nodes, {E} edges: beyond hsg_res_supported")
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        L, M = self.sent_len, self.label_len
        # every active view's running offsets, summed on the host from the kept counts, ride behind
        # the pick list in one small pinned copy, not waited for (the pinned block is recycled
        # stream-safely)
        host = {v: v.offsets(lib, slots, tot) for v in sorted(active, key=lambda v: v.checked)}
        flat, cuts = pack_parts([slots] + [a for v in active for a in host[v]])
        pieces = piece_params()
        with torch.cuda.device(dev):
            both = torch.from_numpy(flat).pin_memory().to(dev, non_blocking=True)
            pick, *arrived = [both[c] for c in cuts]
            offs = new(NFAM * (B + 1), i64)
            st = _lib.stream_of(offs)
            cs = ctypes.byref(self._cstruct)
            p = _lib.ptr
            _lib.check(lib.hsg_res_offsets(cs, B, p(pick), p(offs), st), "hsg_res_offsets")
            nd = dict(unit=new(n, f32), dtype=new(n, f32), id=new(n, i64), words=new((n, L), i64),
                      position=new((n, 1), i64), label=new((n, M), i64))
            src, dst = new(E, i64), new(E, i64)
            ed = dict(tffrac=new(E, i64), dtype=new(E, f32))
            _lib.check(lib.hsg_res_graph(cs, B, p(pick), p(offs), n, E, p(nd["unit"]), p(nd["dtype"]), p(nd["id"]),
                                         p(nd["words"]), p(nd["position"]), p(nd["label"]), p(src), p(dst),
                                         p(ed["tffrac"]), p(ed["dtype"]), st), "hsg_res_graph")
            G = ResidentBatch()
            G._n, G.device = n, dev
            G._nframe, G._ef = Frame(n, dev), Frame(E, dev)
            G._nframe.cols, G._ef.cols = nd, ed
            G._dev_src, G._dev_dst = src, dst
            G.batch_size = B
            G.batch_num_nodes = self.counts[slots, NODE].tolist()
            G.batch_num_edges = self.counts[slots, EDGE].tolist()
            G._origin = (self, slots)
            G._h_src = G._h_dst = None                 # formed from the store on first use
            G._host_cols.update(self._host_node_columns(slots))
            G.resident_work_lists = {}
            b = SimpleNamespace(store=self, G=G, lib=lib, cs=cs, slots=slots, tot=tot, pick=pick, offs=offs, st=st,
                                new=new, glen=self.counts[slots, SENT].tolist())     # the batch, as the views see it
            for q, kind in enumerate(HOT_KINDS):
                ns, ndst, nt = int(tot[SRC(q)]), int(tot[DST(q)]), int(tot[TYP(q)])
                d = dict(indptr=new(ndst + 1, i32), src=new(nt, i32), tf=new(nt, torch.uint8), eid=new(nt, i64),
                         phantom=new(ndst, i32), cindptr=new(ns + 1, i32), cdst=new(nt, i32), cperm=new(nt, i32),
                         src_nodes=new(ns, i64), dst_nodes=new(ndst, i64))
                _lib.check(lib.hsg_res_relation(cs, q, B, p(pick), p(offs), ns, ndst, nt,
                                                *[p(d[k]) for k in REL_ARRAYS], st), "hsg_res_relation")
                lng = self.longest[slots, q].max(0)
                need = needs_work_list(ndst, nt, int(lng[0]), *pieces) or needs_work_list(ns, nt, int(lng[1]), *pieces)
                G.resident_work_lists[kind] = need
                if need and not any(v.work_lists(b, q, d, ns, ndst, nt, pieces) for v in active
                                    if hasattr(v, "work_lists")):
                    attach_work_lists(d, ns, ndst, nt)         # today's path, with its read-back
                G._rel_cache[("rel", kind, str(dev))] = Relation.on_device(kind, ns, ndst, d, E)
            for v in active:                            # each view gets its own slices of the copy back
                v.assemble(b, host[v], arrived[:len(host[v])])
                del arrived[:len(host[v])]
            # the launches above read pick and offs after this returns: the allocator keeps a
            # freed block for later work of the SAME stream, so dropping them here is safe
        if self.eval_words is not None:
            G.eval_words = [w for s in slots for w in self.eval_words[s]]
        return G, [self.indices[s] for s in slots]


class ResidentLoader:
    """Iterates ``(G, index)`` like ``DataLoader(dataset, batch_size, shuffle, collate_fn=
    graph_collate_fn)``, from a :class:`DocumentStore`.  The permutation is drawn on the host
    from ``generator``; ``index`` holds dataset indices; ``model_view``, ``doc_view`` and
    ``eval_view`` are :meth:`DocumentStore.batch`'s."""

    def __init__(self, store, batch_size, shuffle=False, generator=None, drop_last=False, model_view=None,
                 doc_view=None, eval_view=None):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.store, self.batch_size, self.shuffle = store, int(batch_size), shuffle
        self.generator, self.drop_last, self.model_view, self.doc_view = generator, drop_last, model_view, doc_view
        self.eval_view = eval_view

    def __len__(self):
        n = len(self.store)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def batches(self):
        """The dataset indices of every batch of one epoch, before the sort by length."""
        n = len(self.store)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else range(n)
        picks = [self.store.indices[s] for s in order]
        out = [picks[i:i + self.batch_size] for i in range(0, n, self.batch_size)]
        if self.drop_last and out and len(out[-1]) < self.batch_size:
            out.pop()
        return out

    def __iter__(self):
        # a flag left at None is not passed (the store's default): whatever has the store's ``batch(idx)`` serves
        kw = {k: getattr(self, k) for k in ("model_view", "doc_view", "eval_view") if getattr(self, k) is not None}
        for idx in self.batches():
            yield self.store.batch(idx, **kw)
