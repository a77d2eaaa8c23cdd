"""The model glue on native kernels (C ABI: include/hsg_model.h, csrc/hsg_model.hip).

Reference: what HSumGraph / HSumDocGraph compute around the two sentence encoders and
the WSWGAT stack --

* :func:`sent_features` (HiGraph.py:130-132, 141, 160, 96): position embedding + add +
  ``cnn_proj``, ``lstm_proj``, the ``cat`` and ``n_feature_proj`` in one launch;
* :func:`doc_init` (HiGraph.py:231-244, 202, 207): the per-document mean of the sentence
  features, ``dn_feature_proj`` and the supernode gather in one launch;
* :func:`sent_logits` (HiGraph.py:108, 219-227): ``wh`` over the supernode state, for
  HDSG without forming the per-sentence concat.

Each is ONE autograd node.  Parameters are read from the ``nn.Linear`` modules at every
call (nothing derived from a parameter is kept between calls), so state_dict keys and
checkpoints do not change.  The backward launches one row-parallel kernel per node; the
weight gradients of :func:`sent_features` are :func:`hetersumgraph_amd.dense.gemm` with
``dtype="f32"`` and its bias gradients one :class:`hetersumgraph_amd.reduce.SlabBatch`
launch.  All arithmetic is exact fp32 in fixed orders, whatever the process-wide GEMM
mode: two runs are bitwise equal.  No fallback: the functions raise where
:func:`native_ok` is false (HSumGraph.forward asks first).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, load, ptr, stream_of
from .dense import gemm
from .reduce import SlabBatch


def _i32(arr, device):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(device)


def _csr(keys, vals, n):
    """(ptr [n + 1], vals in ascending key, ties in list order)."""
    order = np.argsort(keys, kind="stable")
    p = np.zeros(n + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(keys, minlength=n))
    return p, vals[order]


class HeadLayout:
    """Device index lists of one HDSG batch, built on the host once per graph.

    From the sentence->doc pair list ``(pair_s, pair_d)`` (duplicates kept, any order), the
    supernode order ``super_pos`` (a row of ``cat([sentences, docs])`` per supernode) and
    the per-sentence supernode rows ``sent_super`` / ``doc_super``: the pair list's CSR
    (doc -> sentences) and CSC (sentence -> docs) forms, the inverse of ``super_pos``, and
    the inverse lists of ``sent_super`` and ``doc_super``.  ``ok`` is False for a layout the
    kernels do not take (a doc or a sentence without a supernode row)."""

    def __init__(self, pair_s, pair_d, n_s, n_docs, super_pos, sent_super, doc_super, inv_cnt, device):
        ps, pd = np.asarray(pair_s, np.int64), np.asarray(pair_d, np.int64)
        pos = np.asarray(super_pos, np.int64)
        ss, dsup = np.asarray(sent_super, np.int64), np.asarray(doc_super, np.int64)
        self.n_s, self.n_docs, self.n_super = int(n_s), int(n_docs), len(pos)
        n_super = self.n_super
        doc_ptr, doc_sent = _csr(pd, ps, n_docs)
        sent_ptr, sent_doc = _csr(ps, pd, n_s)
        row_of = np.full(n_s + n_docs, -1, np.int64)
        row_of[pos] = np.arange(n_super)
        self.ok = bool(n_docs > 0 and n_s > 0 and (row_of >= 0).all() and len(ss) == n_s and len(dsup) == n_s
                       and (ss >= 0).all() and (dsup >= 0).all()
                       and len(np.unique(pos)) == n_super)
        sup_sent = np.full(n_super, -1, np.int64)
        sup_ptr, sup_list = np.zeros(n_super + 1, np.int64), np.zeros(0, np.int64)
        if self.ok:
            sup_sent[ss] = np.arange(n_s)
            sup_ptr, sup_list = _csr(dsup, np.arange(n_s), n_super)
        self.super_src = _i32(np.where(pos < n_s, pos, -(pos - n_s + 1)), device)
        self.doc_ptr, self.doc_sent = _i32(doc_ptr, device), _i32(doc_sent, device)
        self.sent_ptr, self.sent_doc = _i32(sent_ptr, device), _i32(sent_doc, device)
        self.sent_row, self.doc_row = _i32(row_of[:n_s], device), _i32(row_of[n_s:], device)
        self.sent_super, self.doc_super = _i32(ss, device), _i32(dsup, device)
        self.sup_sent, self.sup_ptr, self.sup_list = _i32(sup_sent, device), _i32(sup_ptr, device), _i32(sup_list, device)
        self.inv_cnt = torch.as_tensor(inv_cnt, dtype=torch.float32).to(device).contiguous()

    # the int32 lists with their lengths as (n_s, n_docs, n_super, pairs, 1) coefficients
    INT_LISTS = {"super_src": (0, 0, 1, 0, 0), "doc_ptr": (0, 1, 0, 0, 1), "doc_sent": (0, 0, 0, 1, 0),
                 "sent_ptr": (1, 0, 0, 0, 1), "sent_doc": (0, 0, 0, 1, 0), "sent_row": (1, 0, 0, 0, 0),
                 "doc_row": (0, 1, 0, 0, 0), "sent_super": (1, 0, 0, 0, 0), "doc_super": (1, 0, 0, 0, 0),
                 "sup_sent": (0, 0, 1, 0, 0), "sup_ptr": (0, 0, 1, 0, 1), "sup_list": (1, 0, 0, 0, 0)}

    @classmethod
    def prebuilt(cls, n_s, n_docs, n_super, inv_cnt, **lists):
        """A complete layout (``ok``) from index lists already on the device: what the
        constructor builds, assembled elsewhere (the resident store's doc view,
        include/hsg_resident_hdsg.h).  ``lists``: every name of :attr:`INT_LISTS`, int32."""
        lay = cls.__new__(cls)
        lay.n_s, lay.n_docs, lay.n_super, lay.ok = int(n_s), int(n_docs), int(n_super), True
        if set(lists) != set(cls.INT_LISTS) or lay.n_s < 1 or lay.n_docs < 1 or lay.n_super != lay.n_s + lay.n_docs:
            raise ValueError("HeadLayout.prebuilt: every index list of a layout whose supernodes are its "
                             "sentences and doc nodes")
        dims = (lay.n_s, lay.n_docs, lay.n_super, lists["doc_sent"].numel(), 1)
        for k, coef in cls.INT_LISTS.items():
            t = lists[k]
            n = sum(c * d for c, d in zip(coef, dims))
            if t.dtype != torch.int32 or t.device != inv_cnt.device or tuple(t.shape) != (n,) or not t.is_contiguous():
                raise ValueError(f"HeadLayout.prebuilt: '{k}' is not a contiguous int32 [{n}] on the layout's device")
            setattr(lay, k, t)
        if inv_cnt.dtype != torch.float32 or tuple(inv_cnt.shape) != (lay.n_docs,) or not inv_cnt.is_contiguous():
            raise ValueError("HeadLayout.prebuilt: inv_cnt is not a contiguous float32 [n_docs]")
        lay.inv_cnt = inv_cnt
        return lay


_SUPPORTED = {}


def _supported(name, *dims) -> bool:
    """``hsg_<name>_supported(*dims)``, asked once per dimension set (a pure function of
    integers: nothing of a parameter's value is kept)."""
    key = (name,) + dims
    ok = _SUPPORTED.get(key)
    if ok is None:
        ok = _SUPPORTED[key] = bool(getattr(load(), f"hsg_{name}_supported")(*dims))
    return ok


def rows_per_block() -> int:
    """Rows of one block of the sentence-feature kernels (hsg_sentfeat_rows)."""
    return int(load().hsg_sentfeat_rows())


def _f32(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def _weight_ok(w, shape):
    return (_f32(w) and tuple(w.shape) == tuple(shape) and w.is_contiguous() and w.data_ptr() % 16 == 0)


def native_ok(model, rows=None) -> bool:
    """Whether the native glue covers a forward of ``model`` (HSumGraph / HSumDocGraph),
    and, when given, the sentence rows ``rows`` (the n-gram features): fp32 ROCm tensors,
    dimensions the kernels take (hsg_*_supported), biases where the reference has them and
    none where it has none, HSG_CHECK_NAN off (its assertions live on the torch path)."""
    from .module.GATLayer import CHECK_NAN
    if CHECK_NAN or (rows is not None and not (_f32(rows) and rows.dim() == 2)):
        return False
    lin = torch.nn.Linear
    c, l, nf, wh = (getattr(model, k, None) for k in ("cnn_proj", "lstm_proj", "n_feature_proj", "wh"))
    if not all(isinstance(m, lin) for m in (c, l, nf, wh)):
        return False
    E, Fn, Lw, Hs = c.in_features, c.out_features, l.in_features, nf.out_features
    if (rows is not None and rows.shape[1] != E) or c.bias is None or l.bias is None or nf.bias is not None or wh.bias is None:
        return False
    pe = getattr(model, "sent_pos_embed", None)
    if not (isinstance(pe, torch.nn.Embedding) and _f32(pe.weight) and pe.weight.is_contiguous()
            and pe.weight.shape[1] == E and not pe.weight.requires_grad):
        return False
    dn = getattr(model, "dn_feature_proj", None)
    W = 2 * Hs if dn is not None else Hs
    if not (_weight_ok(c.weight, (Fn, E)) and _weight_ok(l.weight, (Fn, Lw)) and _weight_ok(nf.weight, (Hs, 2 * Fn))
            and _weight_ok(wh.weight, (2, W)) and _f32(c.bias) and _f32(l.bias) and _f32(wh.bias)):
        return False
    if not (_supported("sentfeat", E, Fn, Lw, Hs) and _supported("logits", Hs)):
        return False
    if dn is not None:
        if not (isinstance(dn, lin) and dn.bias is None and _weight_ok(dn.weight, (Hs, Hs))
                and _supported("docinit", Hs)):
            return False
    return True


def _rowmajor(t):
    return t if t.stride(-1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


# --------------------------------------------------------------------- sentence features
class _SentFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ngram, pos, P, L, Wc, bc, Wl, bl, Wn):
        lib = load()
        ngram, L = _rowmajor(ngram.detach()), _rowmajor(L.detach())
        n, E = ngram.shape
        Fn, Lw, Hs = Wc.shape[0], Wl.shape[1], Wn.shape[0]
        need = ctx.needs_input_grad
        X = ngram.new_empty(n, E) if need[4] else None
        F = ngram.new_empty(n, 2 * Fn)
        S = ngram.new_empty(n, Hs)
        check(lib.hsg_sentfeat_fwd(n, E, Fn, Lw, Hs, P.shape[0], ptr(ngram), ngram.stride(0), ptr(pos), ptr(P), ptr(L),
                                   L.stride(0), ptr(Wc), ptr(bc), ptr(Wl), ptr(bl), ptr(Wn), ptr(X),
                                   E, ptr(F), 2 * Fn, ptr(S), Hs, stream_of(ngram)), "hsg_sentfeat_fwd")
        ctx.save_for_backward(X, L if need[6] else None, F if need[8] else None, Wc, Wl, Wn)
        return S

    @staticmethod
    def backward(ctx, dS):
        lib = load()
        X, L, F, Wc, Wl, Wn = ctx.saved_tensors
        need = ctx.needs_input_grad
        dS = _rowmajor(dS)
        n, Hs = dS.shape
        (Fn, E), Lw = Wc.shape, Wl.shape[1]
        dF = dS.new_empty(n, 2 * Fn)
        dngram = dS.new_empty(n, E) if need[0] else None
        dL = dS.new_empty(n, Lw) if need[3] else None
        check(lib.hsg_sentfeat_bwd(n, E, Fn, Lw, Hs, ptr(dS), dS.stride(0), ptr(Wc), ptr(Wl), ptr(Wn), ptr(dF), 2 * Fn,
                                   ptr(dngram), E, ptr(dL), Lw, stream_of(dS)), "hsg_sentfeat_bwd")
        zero = n == 0
        dWc = dWl = dWn = dbc = dbl = None
        if need[4]:
            dWc = torch.zeros_like(Wc) if zero else gemm(dF[:, :Fn], X, a_t=True, dtype="f32")
        if need[6]:
            dWl = torch.zeros_like(Wl) if zero else gemm(dF[:, Fn:], L, a_t=True, dtype="f32")
        if need[8]:
            dWn = torch.zeros_like(Wn) if zero else gemm(dS, F, a_t=True, dtype="f32")
        if need[5] or need[7]:
            db = dS.new_zeros(2 * Fn) if zero else dS.new_empty(2 * Fn)
            red = SlabBatch()
            red.add("db", db, 2 * Fn, 2 * Fn, 0, 1.0, False, dF, n)
            red.flush()
            dbc, dbl = (db[:Fn] if need[5] else None), (db[Fn:] if need[7] else None)
        return dngram, None, None, dL, dWc, dbc, dWl, dbl, dWn


def sent_features(ngram, pos, P, L, cnn_proj, lstm_proj, n_feature_proj):
    """``n_feature_proj(cat([cnn_proj(ngram + P[pos]), lstm_proj(L)], 1))`` -> [n, Hs].

    ngram [n, E], pos int64 [n], P [n_pos, E] (the frozen sinusoid table), L [n, Lw] (the
    LSTM output rows; a strided view is read in place).  A position outside
    ``[0, n_pos)`` gives that row NaN instead of an out-of-range read."""
    if not (_f32(ngram) and _f32(L) and _f32(P) and P.is_contiguous() and pos.dtype == torch.int64 and pos.is_cuda):
        raise RuntimeError("sent_features: fp32 ROCm tensors and int64 positions only (no fallback)")
    Wc, Wl, Wn = cnn_proj.weight, lstm_proj.weight, n_feature_proj.weight
    if not _supported("sentfeat", Wc.shape[1], Wc.shape[0], Wl.shape[1], Wn.shape[0]):
        raise RuntimeError("sent_features: dimensions hsg_sentfeat_supported does not cover (no fallback)")
    if ngram.shape[0] != L.shape[0] or ngram.shape[0] != pos.numel():
        raise ValueError("sent_features: row counts differ")
    return _SentFeatures.apply(ngram, pos.contiguous().view(-1), P.detach(), L, Wc, cnn_proj.bias, Wl, lstm_proj.bias, Wn)


# ------------------------------------------------------------------------ doc-node init
class _DocInit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, lay, Wd):
        lib = load()
        S = _rowmajor(S.detach())
        Hs = S.shape[1]
        mean = S.new_empty(lay.n_docs, Hs)
        init = S.new_empty(lay.n_super, Hs)
        check(lib.hsg_docinit_fwd(lay.n_s, lay.n_docs, lay.n_super, Hs, ptr(S), S.stride(0), ptr(lay.super_src),
                                  ptr(lay.doc_ptr), ptr(lay.doc_sent), ptr(lay.inv_cnt), ptr(Wd), ptr(mean), ptr(init),
                                  Hs, stream_of(S)), "hsg_docinit_fwd")
        ctx.save_for_backward(mean, Wd)
        ctx.lay = lay
        return init

    @staticmethod
    def backward(ctx, dInit):
        lib = load()
        mean, Wd = ctx.saved_tensors
        lay, need = ctx.lay, ctx.needs_input_grad
        dInit = _rowmajor(dInit)
        Hs = dInit.shape[1]
        dS = dInit.new_empty(lay.n_s, Hs) if need[0] else None
        dWd = dInit.new_empty(Hs, Hs) if need[2] else None
        check(lib.hsg_docinit_bwd(lay.n_s, lay.n_docs, lay.n_super, Hs, ptr(dInit), dInit.stride(0), ptr(lay.sent_row),
                                  ptr(lay.doc_row), ptr(lay.sent_ptr), ptr(lay.sent_doc), ptr(lay.inv_cnt), ptr(Wd),
                                  ptr(mean), ptr(dS), Hs, ptr(dWd), stream_of(dInit)), "hsg_docinit_bwd")
        return dS, None, dWd


def doc_init(S, lay: HeadLayout, dn_feature_proj):
    """The whole supernode initial state [n_super, Hs]: a sentence row is its row of S, a
    doc row ``dn_feature_proj(mean of its sentences' rows of S)``."""
    if not (_f32(S) and lay.ok and S.shape[0] == lay.n_s and _supported("docinit", S.shape[1])):
        raise RuntimeError("doc_init: fp32 ROCm rows, Hs = 64 and a complete layout only (no fallback)")
    return _DocInit.apply(S, lay, dn_feature_proj.weight)


# ----------------------------------------------------------------------- sentence logits
class _SentLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, lay, Wh, bh):
        lib = load()
        state = _rowmajor(state.detach())
        n_super, Hs = state.shape
        n = lay.n_s if lay is not None else n_super
        logits = state.new_empty(n, 2)
        check(lib.hsg_logits_fwd(n, Hs, n_super, ptr(state), state.stride(0), ptr(lay.sent_super) if lay else None,
                                 ptr(lay.doc_super) if lay else None, ptr(Wh), ptr(bh), ptr(logits), stream_of(state)),
              "hsg_logits_fwd")
        need = ctx.needs_input_grad
        ctx.save_for_backward(state if (need[2] or need[3]) else None, Wh)
        ctx.lay, ctx.shape = lay, (n, n_super, Hs)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = load()
        state, Wh = ctx.saved_tensors
        lay, need = ctx.lay, ctx.needs_input_grad
        n, n_super, Hs = ctx.shape
        dlogits = dlogits.contiguous()
        W = Wh.shape[1]
        want_w = need[2] or need[3]
        dstate = dlogits.new_empty(n_super, Hs) if need[0] else None
        ws = dWh = dbh = None
        if want_w:
            zero = torch.zeros if n == 0 else torch.empty
            ws = dlogits.new_empty(max(lib.hsg_logits_bwd_blocks(n), 1) * (2 * W + 2))
            dWh = zero(2, W, dtype=dlogits.dtype, device=dlogits.device)
            dbh = zero(2, dtype=dlogits.dtype, device=dlogits.device)
        if dstate is not None or want_w:
            check(lib.hsg_logits_bwd(n, Hs, n_super, ptr(dlogits), ptr(state), state.stride(0) if state is not None else Hs,
                                     ptr(lay.sent_super) if lay else None, ptr(lay.doc_super) if lay else None,
                                     ptr(lay.sup_sent) if lay else None, ptr(lay.sup_ptr) if lay else None,
                                     ptr(lay.sup_list) if lay else None, ptr(Wh), ptr(dstate), Hs, ptr(ws), ptr(dWh),
                                     ptr(dbh), stream_of(dlogits)), "hsg_logits_bwd")
        return dstate, None, (dWh if need[2] else None), (dbh if need[3] else None)


def sent_logits(state, lay, wh):
    """``wh`` over the supernode state -> [n, 2].  ``lay`` None (HSG): ``wh(state)``;
    a :class:`HeadLayout` (HDSG): ``wh(cat([state[sent_super], state[doc_super]], 1))``
    without the concatenated matrix."""
    Wh = wh.weight
    if not (_f32(state) and state.dim() == 2 and _supported("logits", state.shape[1]) and wh.bias is not None
            and tuple(Wh.shape) == (2, state.shape[1] * (2 if lay is not None else 1))
            and (lay is None or (lay.ok and lay.n_super == state.shape[0]))):
        raise RuntimeError("sent_logits: fp32 ROCm state and a head of matching width only (no fallback)")
    return _SentLogits.apply(state, lay, Wh, wh.bias)
