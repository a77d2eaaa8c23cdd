"""Guard bands and poison around every buffer the C ABI writes (tests/guard.py).

One table, CASES: entry point -> the cases that call it directly (``_lib.load()``,
``ptr``, ``check``, ``stream_of``).  A case is a function ``fn(lib, mk, **kw)`` that
builds its operands through the allocator ``mk`` and launches once.  The shared body
(``test_guard_bands``) runs it twice:

* guarded: every output and workspace is a ``guarded`` buffer of EXACTLY the extent
  include/hsg.h documents (or exactly what the documented query function returns), with
  a row pitch larger than the column count wherever the entry point takes one; every
  floating-point input is a ``poisoned_input`` -- NaN in its pad columns and before and
  after it (zeros only where the header requires a zero pad: the bf16-A contract);
* plain: the same values in ordinary contiguous ``torch.empty`` / unpadded tensors.

and asserts: the guards are intact (and every input buffer, guards and pad included, is
bitwise what it was), every documented element was written, the pad
columns are untouched (zero where the header promises zero), nothing is NaN or Inf, the
guarded payload is BITWISE the plain run's (the kernels are deterministic: a difference
means the result depends on what lies around the data), and the payload matches the
fp64 restatement of the operation within the tolerance of the entry point's existing
parity test (named at each case).

Adding a case: write ``@case("hsg_entry_point", dict(...), ...)`` over a function that
allocates through ``mk.out`` / ``mk.inp`` / ``mk.scratch`` and returns {output name:
(fp64 reference, atol, rtol)}.  tests/test_guard_coverage.py fails for an entry point
with a writable pointer that has no case here and no reason in its NOT_COVERED.
"""
import ctypes

import numpy as np
import pytest
import torch

# the edge kernels' relations, inputs and fp64 restatements: shared with test_gpu_logit_range.py
from edge_ref import GAT_TOL, N_DST, N_SRC, SEED, ops_tol, r64, relation
from edge_ref import gat_bwd_ref as _gat_bwd_ref
from edge_ref import gat_fwd_inputs as _gat_fwd_inputs
from guard import guarded, poisoned_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = {}                                   # entry point -> [(case id, fn, kwargs)]


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


class Alloc:
    """Operands of one run: guarded + poisoned, or plain contiguous."""

    def __init__(self, guarded_mode):
        self.g = guarded_mode
        self.outs = {}                       # name -> dict(t=view, h=handle | None, pad, mask, finite, scratch)
        self.keep = []                       # the inputs stay allocated until the run was checked
        self.inputs = []                     # guarded run: (whole poisoned buffer, its snapshot before the call)

    def out(self, name, rows, cols, dtype=torch.float32, pitch=None, pad="untouched", mask=None, finite=True,
            plain_pitch=None, init=None, rest=None):
        """An output [rows, cols].  pitch: the guarded run's row pitch (plain: plain_pitch or
        cols).  init: values the call accumulates into (else the buffer starts as the pattern).
        mask: the documented extent; rest="untouched": the header says the elements outside
        it are left as they were (else they carry no promise and are ignored)."""
        if self.g:
            t, h = guarded(rows, cols, dtype, pitch, DEV)
        else:
            pp = plain_pitch or cols
            t, h = torch.empty(rows, pp, dtype=dtype, device=DEV)[:, :cols], None
        if init is not None:
            t.copy_(init)
        self.outs[name] = dict(t=t, h=h, pad=pad, mask=mask, finite=finite, scratch=False, rest=rest)
        return t

    def scratch(self, name, n, dtype=torch.float32):
        """A workspace of exactly n elements whose contents the header does not document:
        only its guards are checked."""
        if n == 0:
            return None
        t = self.out(name, 1, n, dtype)
        self.outs[name]["scratch"] = True
        return t

    def inp(self, t, pitch=None, zero_cols=0, plain_pitch=None):
        """A floating-point input [rows, cols] (or 1-D) with the values of the CPU tensor t."""
        t = t.to(DEV)
        t2 = t if t.dim() == 2 else t.reshape(1, -1)
        if self.g:
            v = poisoned_input(t2, t2.shape[0], t2.shape[1], pitch, zero_cols)
            self.inputs.append((v._base, v._base.clone()))
        else:
            pp = plain_pitch or t2.shape[1]
            buf = torch.zeros(t2.shape[0], pp, dtype=t.dtype, device=DEV)
            buf[:, :t2.shape[1]] = t2
            v = buf[:, :t2.shape[1]]
        self.keep.append(v)
        return v

    def ints(self, t):
        """An integer operand (indices, seeds, offsets): the same plain tensor in both runs."""
        v = t.to(DEV).contiguous()
        self.keep.append(v)
        return v


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def _all_cases():
    return [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs]


def P(t):
    from hetersumgraph_amd._lib import ptr
    return ptr(t)


def ST():
    return torch.cuda.current_stream().cuda_stream


def call(lib, name, *args):
    from hetersumgraph_amd._lib import check
    check(getattr(lib, name)(*args, ST()), name)


def ceil_to(x, m):
    return (x + m - 1) // m * m


def _work_list_post(reld, key, before):
    """The header's promise about a work list after a launch (hsg.h, struct hsg_rel): the
    item words are unchanged, every arrival counter is a multiple of its node's piece
    count (at the first piece's slot; zero elsewhere)."""
    w = reld.dev[key].cpu()
    n = w.numel() // 5
    items, counters = w[:4 * n].view(n, 4), w[4 * n:]
    assert torch.equal(items, before[:4 * n].view(n, 4)), f"{key}: item words changed"
    pieces = {}
    for i in range(n):
        if items[i, 0] < 0:
            pieces[int(items[i, 3])] = pieces.get(int(items[i, 3]), 0) + 1
    assert pieces, f"{key}: the relation has no pieces"
    for i in range(n):
        c = int(counters[i])
        if i in pieces:
            assert c % pieces[i] == 0, f"{key}: counter {c} of item {i} is no multiple of {pieces[i]} pieces"
        else:
            assert c == 0, f"{key}: counter of item {i} (no first piece) is {c}"


GAT_SHAPES = [dict(kind=k, H=H, D=D) for k in ("short", "long") for H, D in ((8, 8), (6, 50))]


@case("hsg_gat_fwd", *GAT_SHAPES)
def c_gat_fwd(lib, mk, kind, H, D):
    """(8, 8): one feature register per lane, (6, 50): five; 'short' one wave per
    destination (k_gat_fwd<.., 1, 7, 2>), 'long' four (k_gat_fwd<.., 4>)."""
    reld, Z, sigma, tau, origin, h_ref, x_ref, ml = _gat_fwd_inputs(kind, H, D)
    HD = H * D
    h, out = mk.out("h", N_DST, HD), mk.out("out", N_DST, HD)
    m, l = mk.out("m", N_DST, H), mk.out("l", N_DST, H)
    call(lib, "hsg_gat_fwd", ctypes.byref(reld.cstruct()), H, D, 0, 0.01, P(mk.inp(Z)), P(mk.inp(sigma)),
         P(mk.inp(tau)), P(mk.inp(origin)), P(h), P(out), P(m), P(l))
    return {"h": (h_ref, *GAT_TOL), "out": (x_ref, *GAT_TOL), **ml}


@case("hsg_gat_fwd_ws", dict(H=8, D=8), dict(H=6, D=50))
def c_gat_fwd_ws(lib, mk, H, D):
    """The CSR work list: pieces of the long destinations written to ws (exactly
    hsg_gat_fwd_ws_floats) and merged by the last arriving block."""
    reld, Z, sigma, tau, origin, h_ref, x_ref, ml = _gat_fwd_inputs("long_wl", H, D)
    HD = H * D
    relp = ctypes.byref(reld.cstruct())
    nws = lib.hsg_gat_fwd_ws_floats(relp, H, D)
    assert nws == (reld.dev["dwork"].numel() // 5) * (HD + 2 * H) > 0
    before = reld.dev["dwork"].cpu().clone()
    h, out = mk.out("h", N_DST, HD), mk.out("out", N_DST, HD)
    m, l = mk.out("m", N_DST, H), mk.out("l", N_DST, H)
    ws = mk.scratch("ws", nws)
    call(lib, "hsg_gat_fwd_ws", relp, H, D, 0, 0.01, P(mk.inp(Z)), P(mk.inp(sigma)), P(mk.inp(tau)),
         P(mk.inp(origin)), P(h), P(out), P(m), P(l), P(ws))
    torch.cuda.synchronize()
    _work_list_post(reld, "dwork", before)
    return {"h": (h_ref, *GAT_TOL), "out": (x_ref, *GAT_TOL), **ml}


def _ld16s(HD):
    c64 = ceil_to(HD, 64)
    return [ceil_to(HD, 8), c64, c64 + 8, c64 + 64]


@case("hsg_gat_fwd_ws16", *[dict(kind=k, H=H, D=D, ld=i) for k in ("short", "long", "long_wl")
                            for H, D in ((8, 8), (6, 50)) for i in range(4)])
def c_gat_fwd_ws16(lib, mk, kind, H, D, ld):
    """x = elu(h) + origin as bf16 rows of pitch ld16 in {ceil8(HD), ceil64(HD), + 8, + 64}:
    the header promises zeros in columns H*D .. ld16 - 1 for every accepted pitch (the
    bf16-A contract), on the whole-node paths ('short', 'long') and the work-list path."""
    reld, Z, sigma, tau, origin, h_ref, x_ref, ml = _gat_fwd_inputs(kind, H, D)
    HD = H * D
    ld16 = _ld16s(HD)[ld]
    relp = ctypes.byref(reld.cstruct())
    nws = lib.hsg_gat_fwd_ws_floats(relp, H, D)
    assert (nws > 0) == (kind == "long_wl")
    before = reld.dev["dwork"].cpu().clone() if nws else None
    x16 = mk.out("x16", N_DST, HD, torch.bfloat16, pitch=ld16, plain_pitch=ld16, pad="zero")
    m, l = mk.out("m", N_DST, H), mk.out("l", N_DST, H)
    ws = mk.scratch("ws", nws)
    call(lib, "hsg_gat_fwd_ws16", relp, H, D, 0, 0.01, P(mk.inp(Z)), P(mk.inp(sigma)), P(mk.inp(tau)),
         P(mk.inp(origin)), None, None, P(m), P(l), P(ws), P(x16), ld16)
    if nws:
        torch.cuda.synchronize()
        _work_list_post(reld, "dwork", before)
    # the fp32 tolerance plus the one RNE rounding of the store, |x16 - x| <= 2^-9 |x| (hsg.h;
    # test_gpu_bf16_x.py::test_gat_fwd_ws16_rows_are_rne_of_fp32 bounds it by 2^-8 |x|)
    return {"x16": (x_ref, GAT_TOL[0], 2.0 ** -8), **ml}


@case("hsg_attn_src_logits", dict(n=1, H=8, D=8), dict(n=97, H=8, D=8), dict(n=97, H=6, D=50))
def c_attn_src_logits(lib, mk, n, H, D):
    Z, a1 = r64(n, H * D), r64(H, D, scale=0.3)
    sigma = mk.out("sigma", n, H)
    call(lib, "hsg_attn_src_logits", n, H, D, P(mk.inp(Z)), P(mk.inp(a1)), P(sigma))
    ref = (Z.double().view(n, H, D) * a1.double()).sum(-1)
    return {"sigma": (ref, *GAT_TOL)}            # part of test_gat_aggregate_matches_op_restatement's chain


# ------------------------------------------------------------------------------------
# edge backward.  The fp64 restatement (edge_ref.gat_bwd_ref) is the header's formulas on the
# forward's fp64 (h, m, l); tolerance: test_gpu_ops.py::test_gat_aggregate_matches_op_restatement --
# 2e-5 * max(1, |ref|_max) per gradient.
GB = [dict(kind=k, H=H, D=D) for k in ("short", "long") for H, D in ((8, 8), (6, 50))]


@case("hsg_gat_bwd_dst", *[dict(c, om=om) for c in GB for om in (1, 0)])
def c_gat_bwd_dst(lib, mk, kind, H, D, om):
    """om 1: G = dOut * elu'(h) (out = elu(h) + origin); om 0: no origin, G = dOut."""
    reld, v, r, E = _gat_bwd_ref(kind, H, D, om=om)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    nb = lib.hsg_gat_bwd_blocks(relp)
    G, dpre, dtp = mk.out("G", N_DST, HD), mk.out("dpre", E, H), mk.out("dtau_part", nb, 11 * H)
    call(lib, "hsg_gat_bwd_dst", relp, H, D, 0, om, 0.01, P(mk.inp(v["Z"])), P(mk.inp(v["sigma"])), P(mk.inp(v["tau"])),
         P(mk.inp(r["h"].float())), P(mk.inp(r["m"].float())), P(mk.inp(r["l"].float())), P(mk.inp(v["dout"])), P(G),
         P(dpre), P(dtp))
    return {"G": (r["G"], *ops_tol(r["G"])), "dpre": (r["dpre"], *ops_tol(r["dpre"])),
            "dtau_part": (("colsum", r["dtau"]), *ops_tol(r["dtau"]))}


@case("hsg_gat_bwd_dst_noh")
def c_gat_bwd_dst_noh(lib, mk):
    """The forward without h (short segments, D > 16): elu'(h) from x - origin."""
    H, D = 6, 50
    reld, v, r, E = _gat_bwd_ref("short", H, D)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    assert lib.hsg_gat_bwd_dst_noh_supported(relp, H, D)
    nb = lib.hsg_gat_bwd_blocks(relp)
    G, dpre, dtp = mk.out("G", N_DST, HD), mk.out("dpre", E, H), mk.out("dtau_part", nb, 11 * H)
    call(lib, "hsg_gat_bwd_dst_noh", relp, H, D, 0, 0.01, P(mk.inp(v["Z"])), P(mk.inp(v["sigma"])), P(mk.inp(v["tau"])),
         P(mk.inp(r["x"].float())), P(mk.inp(v["origin"])), P(mk.inp(r["m"].float())), P(mk.inp(r["l"].float())),
         P(mk.inp(v["dout"])), P(G), P(dpre), P(dtp))
    # elu'(h) = x - origin + 1 carries the fp32 rounding of x (|x| ~ 4): 2^-24 |x| |dOut| on G
    return {"G": (r["G"], *ops_tol(r["G"])), "dpre": (r["dpre"], *ops_tol(r["dpre"])),
            "dtau_part": (("colsum", r["dtau"]), *ops_tol(r["dtau"]))}


@case("hsg_gat_bwd_dst_g")
def c_gat_bwd_dst_g(lib, mk):
    H, D = 6, 50
    reld, v, r, E = _gat_bwd_ref("short", H, D)
    relp = ctypes.byref(reld.cstruct())
    assert lib.hsg_gat_bwd_dst_noh_supported(relp, H, D)
    nb = lib.hsg_gat_bwd_blocks(relp)
    dpre, dtp = mk.out("dpre", E, H), mk.out("dtau_part", nb, 11 * H)
    call(lib, "hsg_gat_bwd_dst_g", relp, H, D, 0, 0.01, P(mk.inp(v["Z"])), P(mk.inp(v["sigma"])), P(mk.inp(v["tau"])),
         P(mk.inp(r["m"].float())), P(mk.inp(r["l"].float())), P(mk.inp(r["G"].float())), P(dpre), P(dtp))
    return {"dpre": (r["dpre"], *ops_tol(r["dpre"])), "dtau_part": (("colsum", r["dtau"]), *ops_tol(r["dtau"]))}


@case("hsg_gat_bwd_src", *[dict(c, full=f) for c in GB for f in (1, 0)])
def c_gat_bwd_src(lib, mk, kind, H, D, full):
    """full: a1 folded into dZ, dsigma and the da1 partials written; else dZ alone."""
    reld, v, r, E = _gat_bwd_ref(kind, H, D)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    nb = lib.hsg_gat_bwd_src_blocks(relp)
    dZ = mk.out("dZ", N_SRC, HD)
    dsig = mk.out("dsigma", N_SRC, H) if full else None
    da1p = mk.out("da1_part", nb, HD) if full else None
    call(lib, "hsg_gat_bwd_src", relp, H, D, 0, 0.01, P(mk.inp(v["sigma"])), P(mk.inp(v["tau"])),
         P(mk.inp(r["m"].float())), P(mk.inp(r["l"].float())), P(mk.inp(r["G"].float())), P(mk.inp(r["dpre"].float())),
         P(mk.inp(v["a1"])) if full else None, P(mk.inp(v["Z"])) if full else None, P(dZ), P(dsig), P(da1p))
    if not full:
        return {"dZ": (r["dZ0"], *ops_tol(r["dZ0"]))}
    return {"dZ": (r["dZ"], *ops_tol(r["dZ"])), "dsigma": (r["dsigma"], *ops_tol(r["dsigma"])),
            "da1_part": (("colsum", r["da1"]), *ops_tol(r["da1"]))}


def _src_g(lib, mk, entry, kind, H, D, g_bf16=0, dsig=1):
    reld, v, r, E = _gat_bwd_ref(kind, H, D, g_bf16=bool(g_bf16))
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    assert lib.hsg_gat_bwd_src_g_supported(relp, H, D)
    wide = D >= 32
    nb = lib.hsg_gat_bwd_src_g_blocks(relp, H, D)
    rho = r["rho_groups"].reshape(N_DST, -1) if wide else r["rho"]
    groups = (HD + 63) // 64 if wide else 0
    dZ = mk.out("dZ", N_SRC, HD)
    dsigma = mk.out("dsigma", N_SRC, H) if dsig else None
    da1p, dtp = mk.out("da1_part", nb, HD), mk.out("dtau_part", nb, 11 * H)
    Gd = mk.inp(v["G16"]) if g_bf16 else mk.inp(r["G"].float())
    args = [relp, H, D, 0.01, P(mk.inp(v["sigma"])), P(mk.inp(v["tau"])), P(mk.inp(r["m"].float())),
            P(mk.inp(r["l"].float())), P(Gd)] + ([g_bf16] if entry != "hsg_gat_bwd_src_g" else []) + [
        P(mk.inp(rho.float())), groups, P(mk.inp(v["a1"])), P(mk.inp(v["Z"])), P(dZ), P(dsigma), P(da1p), P(dtp)]
    before = None
    if entry == "hsg_gat_bwd_src_g_ws":
        nws = lib.hsg_gat_bwd_src_g_ws_floats(relp, H, D)
        assert (nws > 0) == (kind == "long_wl" and wide)
        if nws:
            assert nws == (reld.dev["swork"].numel() // 5) * (HD + H)
            before = reld.dev["swork"].cpu().clone()
        args.append(P(mk.scratch("ws", nws)))
    call(lib, entry, *args)
    if before is not None:
        torch.cuda.synchronize()
        _work_list_post(reld, "swork", before)
    refs = {"dZ": (r["dZ"], *ops_tol(r["dZ"])), "da1_part": (("colsum", r["da1"]), *ops_tol(r["da1"])),
            "dtau_part": (("colsum", r["dtau"]), *ops_tol(r["dtau"]))}
    if dsig:
        refs["dsigma"] = (r["dsigma"], *ops_tol(r["dsigma"]))
    return refs


SRCG = [dict(kind="short", H=8, D=8), dict(kind="long", H=6, D=50)]     # the narrow head-lane kernel, the wide one


@case("hsg_gat_bwd_src_g", *SRCG)
def c_gat_bwd_src_g(lib, mk, kind, H, D):
    return _src_g(lib, mk, "hsg_gat_bwd_src_g", kind, H, D)


@case("hsg_gat_bwd_src_g_io", *SRCG, dict(kind="long", H=6, D=50, g_bf16=1, dsig=0))
def c_gat_bwd_src_g_io(lib, mk, kind, H, D, g_bf16=0, dsig=1):
    return _src_g(lib, mk, "hsg_gat_bwd_src_g_io", kind, H, D, g_bf16, dsig)


@case("hsg_gat_bwd_src_g_ws", *SRCG, dict(kind="long_wl", H=6, D=50), dict(kind="long_wl", H=6, D=50, g_bf16=1, dsig=0))
def c_gat_bwd_src_g_ws(lib, mk, kind, H, D, g_bf16=0, dsig=1):
    """'long_wl': the CSC work list -- pieces of the long sources in ws (exactly
    hsg_gat_bwd_src_g_ws_floats), summed in piece order by the second launch."""
    return _src_g(lib, mk, "hsg_gat_bwd_src_g_ws", kind, H, D, g_bf16, dsig)


# ------------------------------------------------------------------------------------
# attention parameters of one layer application: the W2S-like layer (8 heads x 8, no
# feat_fc bias) and the S2W-like one (6 x 50, with bias), F = 50.  Tolerance:
# test_gpu_ops.py::test_gat_heads_table_matches_restatement -- 2e-5 * max(1, |ref|_max).
LAYERS = [dict(H=8, D=8, bias=0), dict(H=6, D=50, bias=1)]
F_TF = 50


def _layer_params(H, D, bias):
    return dict(attn=r64(H, 3 * D, scale=0.3), wf=r64(H * D, F_TF) / F_TF ** 0.5,
                bf=r64(H, D, scale=0.2) if bias else None)


def _tau_ref(L, T, H, D):
    from test_gpu_ops import tau_table_ref
    bf = L["bf"].double() if L["bf"] is not None else None
    return tau_table_ref(L["attn"].double(), T.double(), L["wf"].double().view(H, D, F_TF), bf, D)


def _tables_out(mk, q, L, T, H, D, refs):
    a1, tau = mk.out(f"a1_{q}", H, D), mk.out(f"tau{q}", 11, H)
    refs[f"a1_{q}"] = (L["attn"][:, :D].double(), 0.0, 0.0)
    t = _tau_ref(L, T, H, D)
    refs[f"tau{q}"] = (t, *ops_tol(t))
    return [P(mk.inp(L["attn"])), P(mk.inp(L["wf"])), P(mk.inp(L["bf"])) if L["bf"] is not None else None, P(a1),
            P(tau)]


@case("hsg_attn_params_fwd", *LAYERS)
def c_attn_params_fwd(lib, mk, H, D, bias):
    L, T, refs = _layer_params(H, D, bias), r64(10, F_TF), {}
    a = _tables_out(mk, 0, L, T, H, D, refs)
    call(lib, "hsg_attn_params_fwd", H, D, F_TF, a[0], a[1], a[2], P(mk.inp(T)), a[3], a[4])
    return refs


def _fwd_pair(lib, mk, with_seed):
    T, refs, args = r64(10, F_TF), {}, []
    for q, lay in enumerate(LAYERS):
        L = _layer_params(**lay)
        args += [lay["H"], lay["D"]] + _tables_out(mk, q, L, T, lay["H"], lay["D"], refs)
    args += [F_TF, P(mk.inp(T))]
    if with_seed:
        seed = mk.out("seed", 1, 1, torch.int64, init=torch.tensor([[41]]))
        snap = mk.out("snap", 1, 1, torch.int64)
        args += [P(seed), P(snap)]
        refs["seed"] = refs["snap"] = (torch.tensor([[42.0]], dtype=torch.float64), 0, 0)
    call(lib, "hsg_attn_params_fwd_pair_seed" if with_seed else "hsg_attn_params_fwd_pair", *args)
    return refs


@case("hsg_attn_params_fwd_pair")
def c_attn_params_fwd_pair(lib, mk):
    return _fwd_pair(lib, mk, False)


@case("hsg_attn_params_fwd_pair_seed")
def c_attn_params_fwd_pair_seed(lib, mk):
    return _fwd_pair(lib, mk, True)


def _attn_bwd_ref(L, T, H, D, dtau, da1):
    """(dattn, dwf, dbf, dT) in fp64 from the summed partials."""
    lv = {k: (v.double().clone().requires_grad_() if v is not None else None) for k, v in L.items()}
    Tl = T.double().clone().requires_grad_()
    from test_gpu_ops import tau_table_ref
    tau = tau_table_ref(lv["attn"], Tl, lv["wf"].view(H, D, F_TF), lv["bf"], D)
    ((tau * dtau.view(11, H)).sum() + (lv["attn"][:, :D] * da1.view(H, D)).sum()).backward()
    return lv["attn"].grad, lv["wf"].grad, lv["bf"].grad if lv["bf"] is not None else None, Tl.grad


def _grad_outs(mk, q, L, T, acc, refs, r, dT=None):
    """dattn / dwf / dbf / dT outputs (accumulate bit 0: the head's, bit 1: dT) and their references."""
    names = [f"dattn{q}", f"dwf{q}", f"dbf{q}", f"dT{q}"]
    like = [L["attn"], L["wf"], L["bf"], T]
    outs = []
    for i, (nm, lk, ref) in enumerate(zip(names, like, r)):
        if lk is None:
            outs.append(None)
            continue
        if i == 3 and dT is not None:
            outs.append(dT)
            continue
        a = bool(acc & (2 if i == 3 else 1))
        init = r64(*lk.shape) if a else None
        outs.append(mk.out(nm, lk.shape[0], lk.shape[1], init=init))
        full = ref + (init.double() if a else 0)
        refs[nm] = (full, *ops_tol(ref))
    return outs


@case("hsg_attn_params_bwd", *[dict(l, acc=a, nt=nt, na=na)
                               for l, a, nt, na in zip(LAYERS * 2, (0, 3, 1, 2), (3, 1, 5, 2), (1, 4, 2, 7))])
def c_attn_params_bwd(lib, mk, H, D, bias, acc, nt, na):
    L, T = _layer_params(H, D, bias), r64(10, F_TF)
    dtp, dap = r64(nt, 11 * H), r64(na, H * D)
    r = _attn_bwd_ref(L, T, H, D, dtp.double().sum(0), dap.double().sum(0))
    refs = {}
    o = _grad_outs(mk, 0, L, T, acc, refs, r)
    ws = mk.scratch("ws", lib.hsg_attn_params_bwd_workspace_floats(H, D))
    call(lib, "hsg_attn_params_bwd", H, D, F_TF, nt, P(mk.inp(dtp)), na, P(mk.inp(dap)), P(mk.inp(L["attn"])),
         P(mk.inp(L["wf"])), P(mk.inp(L["bf"])) if bias else None, P(mk.inp(T)), P(o[0]), P(o[1]), P(o[2]), P(o[3]),
         P(ws), acc)
    return refs


def _stage_rows(lib, H, D):
    n = lib.hsg_attn_params_bwd_workspace_floats(H, D)
    assert n % (11 * H + H * D) == 0
    return n, n // (11 * H + H * D)


@case("hsg_attn_params_stage", *[dict(l, acc=a, nt=nt, na=na)
                                 for l, a, nt, na in zip(LAYERS * 2, (0, 1, 1, 0), (3, 1, 130, 2), (1, 4, 2, 70))])
def c_attn_params_stage(lib, mk, H, D, bias, acc, nt, na):
    """The workspace [rows][11 H] + [rows][H D] (hsg_attn_params_bwd_workspace_floats) receives
    the application's partial slabs, or has them added: its row sums are the slabs' sums."""
    n, rows = _stage_rows(lib, H, D)
    dtp, dap = r64(nt, 11 * H), r64(na, H * D)
    init = r64(1, n) if acc else None
    ws = mk.out("ws", 1, n, init=init)
    call(lib, "hsg_attn_params_stage", H, D, nt, P(mk.inp(dtp)), na, P(mk.inp(dap)), P(ws), acc)
    base = init.double().view(-1) if acc else torch.zeros(n, dtype=torch.float64)
    rt = dtp.double().sum(0) + base[:rows * 11 * H].view(rows, -1).sum(0)
    ra = dap.double().sum(0) + base[rows * 11 * H:].view(rows, -1).sum(0)

    def check_ws(got):
        got = got.double().view(-1)
        for nm, g, r in (("dtau", got[:rows * 11 * H].view(rows, -1).sum(0), rt),
                         ("da1", got[rows * 11 * H:].view(rows, -1).sum(0), ra)):
            tol = 1e-4 + 1e-5 * r.abs()         # test_gpu_gemm.py::test_slab_batch_staged_rows (the same reduction)
            assert bool(((g - r).abs() <= tol).all()), (nm, (g - r).abs().max().item())
    return {"ws": (check_ws, 0, 0)}


@case("hsg_attn_params_finish", *[dict(l, acc=a) for l, a in zip(LAYERS * 2, (0, 3, 2, 1))])
def c_attn_params_finish(lib, mk, H, D, bias, acc):
    L, T = _layer_params(H, D, bias), r64(10, F_TF)
    n, rows = _stage_rows(lib, H, D)
    wsv = r64(1, n)
    dtau = wsv.double().view(-1)[:rows * 11 * H].view(rows, -1).sum(0)
    da1 = wsv.double().view(-1)[rows * 11 * H:].view(rows, -1).sum(0)
    refs = {}
    o = _grad_outs(mk, 0, L, T, acc, refs, _attn_bwd_ref(L, T, H, D, dtau, da1))
    call(lib, "hsg_attn_params_finish", H, D, F_TF, P(mk.inp(wsv)), P(mk.inp(L["attn"])), P(mk.inp(L["wf"])),
         P(mk.inp(L["bf"])) if bias else None, P(mk.inp(T)), P(o[0]), P(o[1]), P(o[2]), P(o[3]), acc)
    return refs


@case("hsg_attn_params_finish_pair", dict(shared=1, a0=0, a1=2), dict(shared=0, a0=3, a1=0), dict(shared=1, a0=3, a1=3))
def c_attn_params_finish_pair(lib, mk, shared, a0, a1):
    """Both layers in one launch; a shared dT takes layer 0's update, then layer 1's."""
    T, refs, args = r64(10, F_TF), {}, []
    dT_shared, dT_ref = None, None
    for q, (lay, acc) in enumerate(zip(LAYERS, (a0, a1))):
        H, D = lay["H"], lay["D"]
        L = _layer_params(**lay)
        n, rows = _stage_rows(lib, H, D)
        wsv = r64(1, n)
        dtau = wsv.double().view(-1)[:rows * 11 * H].view(rows, -1).sum(0)
        da1 = wsv.double().view(-1)[rows * 11 * H:].view(rows, -1).sum(0)
        r = _attn_bwd_ref(L, T, H, D, dtau, da1)
        o = _grad_outs(mk, q, L, T, acc, refs, r, dT=dT_shared if (shared and q == 1) else None)
        if shared and q == 0:
            dT_shared, dT_ref = o[3], refs["dT0"][0]
        elif shared:
            refs["dT0"] = (dT_ref + r[3], *ops_tol(dT_ref + r[3]))
        args += [H, D, P(mk.inp(wsv)), P(mk.inp(L["attn"])), P(mk.inp(L["wf"])),
                 P(mk.inp(L["bf"])) if L["bf"] is not None else None, P(o[0]), P(o[1]), P(o[2]), P(o[3]), acc]
    call(lib, "hsg_attn_params_finish_pair", *args, F_TF, P(mk.inp(T)))
    return refs


# ------------------------------------------------------------------------------------
# dense GEMMs.  M in {1, 129}: one short row tile, one full tile plus a row; N = 512 the
# k_gemm13 route, K = 300 / 76 the K tail (K % 32 != 0), N = 300 / 100 padded widths
GEMM_MNK = [(M, N, K) for M in (1, 129) for N, K in ((512, 300), (300, 512), (64, 300), (100, 76))]


def gemm_tol(K):
    """test_gpu_gemm.py::test_layouts / test_psw_layouts: 1e-5 * max(1, sqrt(K)) * 4, absolute."""
    return 1e-5 * max(1.0, K ** 0.5) * 4


def _gemm_operands(mk, M, N, K, ak, bk):
    A, B = r64(M, K), r64(K, N)
    Ad = mk.inp(A if ak else A.t().contiguous(), pitch=ceil_to(K if ak else M, 4) + 4,
                plain_pitch=ceil_to(K if ak else M, 4))
    Bd = mk.inp(B.t().contiguous() if bk else B, pitch=ceil_to(K if bk else N, 4) + 4,
                plain_pitch=ceil_to(K if bk else N, 4))
    return A, B, Ad, Bd


GEMM_CASES = [
    *[dict(M=M, N=N, K=K, ak=1, bk=1, sp=1, epi=0) for M, N, K in GEMM_MNK],
    *[dict(M=129, N=100, K=76, ak=ak, bk=bk, sp=1, epi=0) for ak, bk in ((1, 0), (0, 0), (0, 1))],
    *[dict(M=129, N=300, K=512, ak=ak, bk=bk, sp=sp, epi=0) for ak, bk in ((1, 1), (0, 0)) for sp in (0, 3)],
    dict(M=1, N=64, K=300, ak=1, bk=1, sp=0, epi=0), dict(M=129, N=100, K=76, ak=1, bk=0, sp=3, epi=0),
    dict(M=129, N=300, K=76, ak=1, bk=1, sp=1, epi=1), dict(M=129, N=100, K=300, ak=1, bk=0, sp=1, epi=2),
    dict(M=129, N=512, K=300, ak=1, bk=1, sp=1, epi=3), dict(M=1, N=100, K=76, ak=1, bk=1, sp=1, epi=3),
    # the sentence CNN's GEMMs (cnn.py): Y = X Wall^T at N = 1350 into a pitched Y, the split-K dWall = dY^T X
    # with both operands M/N-contiguous, dX = dY Wall
    dict(M=35, N=1350, K=300, ak=1, bk=1, sp=1, epi=4), dict(M=1350, N=300, K=35, ak=0, bk=0, sp=2, epi=4),
    dict(M=35, N=300, K=1350, ak=1, bk=0, sp=0, epi=4)]


def _gemm(lib, mk, entry, bf16, M, N, K, ak, bk, sp, epi):

    """epi 0: store + bias + relu, 1: relu' mask, 2: accumulate into C, 3: store with
    colsum_part [hsg_gemm_row_tiles][N], 4: plain store; sp: 1 unsplit, 0 the automatic plan
    (which splits every shape chosen for it), 2 / 3 explicit (workspace of exactly
    hsg_gemm_workspace_floats).  bf16 (hsg_gemm_bf16): the fp64 product of the RNE-rounded
    operands, test_gpu_gemm.py::test_bf16_layouts' bound (the same 1e-5 * max(1, sqrt(K)) * 4)."""
    A, B, Ad, Bd = _gemm_operands(mk, M, N, K, ak, bk)
    ldc = N + 3
    ref = A.bfloat16().double() @ B.bfloat16().double() if bf16 else A.double() @ B.double()
    bias = aux = None
    epi_c, relu = 0, 0
    init = None
    if epi in (0, 3):
        bias, relu = r64(N), int(epi == 0)
        ref = ref + bias.double()
        ref = torch.relu(ref) if relu else ref
    elif epi == 1:
        auxv = r64(M, N)
        aux, epi_c = mk.inp(auxv, pitch=N + 5), 1
        ref = ref * (auxv.double() > 0)
    elif epi == 2:
        init, epi_c = r64(M, N), 2
        ref = ref + init.double()
    C = mk.out("C", M, N, pitch=ldc, init=init)
    nws = lib.hsg_gemm_workspace_floats(M, N, K, sp)
    eff = sp if sp else lib.hsg_gemm_auto_splits(M, N, K)
    assert eff > 1 or sp == 1, "the automatic plan does not split this shape: the case would run unsplit"
    assert nws == (eff * M * N if eff > 1 else 0)
    ws = mk.scratch("ws", nws)
    refs = {"C": (ref, gemm_tol(K), 0.0)}
    part = None
    if epi == 3:
        rt = lib.hsg_gemm_row_tiles(M, N, K, 1)
        part = mk.out("colsum_part", rt, N)
        pr = torch.stack([ref[64 * t:64 * (t + 1)].sum(0) for t in range(rt)])
        refs["colsum_part"] = (pr, 1e-3, 1e-6)      # test_gpu_gemm.py::test_psw_epilogues_and_colsums
    if epi == 2:
        aux = C
    call(lib, entry, M, N, K, P(Ad), Ad.stride(0), ak, P(Bd), Bd.stride(0), bk, P(C), C.stride(0),
         P(mk.inp(bias)) if bias is not None else None, P(aux), aux.stride(0) if aux is not None else 0, epi_c, relu,
         sp, P(ws), P(part))
    return refs


@case("hsg_gemm_f32", *GEMM_CASES)
def c_gemm_f32(lib, mk, M, N, K, ak, bk, sp, epi):
    return _gemm(lib, mk, "hsg_gemm_f32", False, M, N, K, ak, bk, sp, epi)


@case("hsg_gemm_bf16", *GEMM_CASES)
def c_gemm_bf16(lib, mk, M, N, K, ak, bk, sp, epi):
    """The bf16 GEMM mode's unsplit-weight GEMM: what dense.gemm() calls in that mode (the
    sentence CNN's three GEMMs, the weight gradients outside the batched launch)."""
    return _gemm(lib, mk, "hsg_gemm_bf16", True, M, N, K, ak, bk, sp, epi)


def _slabs(lib, mk, name, M, N, K, ak, bk, sp, bf16):
    A, B, Ad, Bd = _gemm_operands(mk, M, N, K, ak, bk)
    assert lib.hsg_gemm_workspace_floats(M, N, K, sp) == sp * M * N
    ws = mk.out("ws", sp, M * N)                      # workspace[splits][M][N]: every slice's products
    call(lib, name, M, N, K, P(Ad), Ad.stride(0), ak, P(Bd), Bd.stride(0), bk, sp, P(ws))
    a64, b64 = (A.bfloat16().double(), B.bfloat16().double()) if bf16 else (A.double(), B.double())
    kt = (K + 31) // 32
    per = (kt + sp - 1) // sp
    ref = torch.stack([(a64[:, 32 * per * s:32 * per * (s + 1)] @ b64[32 * per * s:32 * per * (s + 1)]).reshape(-1)
                       for s in range(sp)])
    return {"ws": (ref, gemm_tol(K), 0.0)}


SLAB_CASES = [dict(M=M, N=N, K=K, ak=ak, bk=bk, sp=sp) for (M, N, K, ak, bk, sp) in
              ((129, 300, 512, 0, 0, 3), (1, 512, 300, 1, 1, 2), (129, 100, 76, 0, 0, 3), (129, 64, 300, 1, 0, 5))]


@case("hsg_gemm_f32_slabs", *SLAB_CASES)
def c_gemm_f32_slabs(lib, mk, M, N, K, ak, bk, sp):
    return _slabs(lib, mk, "hsg_gemm_f32_slabs", M, N, K, ak, bk, sp, False)


@case("hsg_gemm_bf16_slabs", *SLAB_CASES)
def c_gemm_bf16_slabs(lib, mk, M, N, K, ak, bk, sp):
    # test_gpu_gemm.py::test_psw_bf16_mode_is_the_rounded_product: the fp64 product of the RNE operands
    return _slabs(lib, mk, "hsg_gemm_bf16_slabs", M, N, K, ak, bk, sp, True)


def _arr(ct, xs):
    return (ct * len(xs))(*xs)


@case("hsg_slab_reduce", dict(vec=1), dict(vec=0))
def c_slab_reduce(lib, mk, vec):
    """Two jobs in one launch: (cols, pitch, coff) multiples of 4 (the float4 columns) or
    not; job 0 plain column sums over two segments, job 1 accumulating, scaled and staged
    (out_rows = 3).  test_gpu_gemm.py::test_slab_batch_sums_segments_in_one_launch: rtol 1e-5, atol 1e-4."""
    cols, pitch, coff = ((88, 300), (180, 304), (88, 4)) if vec else ((70, 301), (211, 303), (70, 2))
    rows = [[5, 17], [7]]
    out_rows = [1, 3]
    scale, acc = [1.0, 0.75], [0, 1]
    segs, outs, refs = [], [], {}
    nan = float("nan")
    for q in range(2):
        # a segment row: [coff columns of another job (never read here: NaN) | cols | pad up to pitch (poison)]
        sv = [r64(r, cols[q]) for r in rows[q]]
        for s in sv:
            full = torch.cat([torch.full((s.shape[0], coff[q]), nan), s], 1)
            segs.append(mk.inp(full, pitch=pitch[q], plain_pitch=pitch[q]))
        init = r64(out_rows[q], cols[q]) if acc[q] else None
        outs.append(mk.out(f"out{q}", out_rows[q], cols[q], init=init))
        ref = init.double().clone() if acc[q] else torch.zeros(out_rows[q], cols[q], dtype=torch.float64)
        for s in sv:
            per = (s.shape[0] + out_rows[q] - 1) // out_rows[q]
            for b in range(out_rows[q]):
                ref[b] += scale[q] * s[b * per:(b + 1) * per].double().sum(0)
        refs[f"out{q}"] = (ref, 1e-4, 1e-5)
    i32, f32, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    call(lib, "hsg_slab_reduce", 2, _arr(vp, [P(o) for o in outs]), _arr(i32, cols), _arr(i32, out_rows),
         _arr(i32, pitch), _arr(i32, coff), _arr(f32, scale), _arr(i32, acc),
         _arr(i32, [2, 1]), _arr(vp, [P(s) for s in segs]), _arr(i32, rows[0] + rows[1]))
    return refs


def _wsplit(lib, mk, W, N, K, trans, name="planes", bf16=False):
    """The limb planes [3][Np][Kp] of B = trans ? W^T : W through hsg_wsplit (a guarded
    output of exactly 3 * Np * Kp bf16: zero padded, so every element is written)."""
    np_, kp = ctypes.c_int(), ctypes.c_int()
    lib.hsg_wsplit_dims(N, K, ctypes.byref(np_), ctypes.byref(kp))
    Np, Kp = np_.value, kp.value
    assert Np == ceil_to(N, 128) and Kp == ceil_to(K, 32)
    planes = mk.out(name, 3 * Np, Kp, torch.bfloat16)
    Wd = mk.inp(W, pitch=W.shape[1] + 3)
    i32, vp = ctypes.c_int, ctypes.c_void_p
    call(lib, "hsg_wsplit", 1, _arr(vp, [P(Wd)]), _arr(i32, [N]), _arr(i32, [K]), _arr(i32, [Wd.stride(0)]),
         _arr(i32, [int(trans)]), _arr(vp, [P(planes)]))
    Bm = (W.t() if trans else W).double()
    ref = torch.zeros(3, Np, Kp, dtype=torch.float64)
    rest = Bm.clone()
    for q in range(3):                              # limbs as hsg_gemm_f32's split: RNE of the remainder
        limb = rest.float().bfloat16().double()
        ref[q, :N, :K] = limb
        rest = rest - limb
    return planes, ref.view(3 * Np, Kp), Np, Kp


@case("hsg_wsplit", dict(N=512, K=300, trans=0), dict(N=300, K=512, trans=1), dict(N=100, K=76, trans=0),
      dict(N=64, K=300, trans=1))
def c_wsplit(lib, mk, N, K, trans):
    W = r64(K, N) if trans else r64(N, K)
    _, ref, _, _ = _wsplit(lib, mk, W, N, K, trans)
    return {"planes": (ref, 0.0, 0.0)}               # the limbs are exact roundings: bitwise the restatement


def _psw(lib, mk, entry, M, N, K, epi, plan=None, bf16=False):
    """C = A W^T on the pre-split W [N][K]; epi as c_gemm_f32 (3: colsum_part of
    hsg_gemm_psw_row_tiles rows)."""
    A, W = r64(M, K), r64(N, K)
    planes, _, _, _ = _wsplit(lib, mk, W, N, K, 0)
    Ad = mk.inp(A, pitch=ceil_to(K, 4) + 4, plain_pitch=ceil_to(K, 4))
    a64, w64 = (A.bfloat16().double(), W.bfloat16().double()) if bf16 else (A.double(), W.double())
    ref = a64 @ w64.t()
    bias = aux = part = init = None
    epi_c, relu = 0, 0
    if epi in (0, 3):
        bias, relu = r64(N), int(epi == 0)
        ref = ref + bias.double()
        ref = torch.relu(ref) if relu else ref
    elif epi == 1:
        auxv = r64(M, N)
        aux, epi_c = mk.inp(auxv, pitch=N + 8), 1
        ref = ref * (auxv.double() > 0)
    else:
        init, epi_c = r64(M, N), 2
        ref = ref + init.double()
    C = mk.out("C", M, N, pitch=N + 4, init=init)
    # test_gpu_gemm.py::test_psw_layouts (fp32 mode) / test_psw_bf16_mode_is_the_rounded_product (bf16:
    # 1e-5 * max(1, |ref|_max) * max(1, sqrt(K)))
    tol = 1e-5 * max(1.0, ref.abs().max().item()) * max(1.0, K ** 0.5) if bf16 else gemm_tol(K)
    refs = {"C": (ref, tol, 0.0)}
    if epi == 3:
        rt = lib.hsg_gemm_psw_row_tiles(M, N, K, int(bf16))
        part = mk.out("colsum_part", rt, N)
    if epi == 2:
        aux = C
    args = [M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0), P(mk.inp(bias)) if bias is not None else None,
            P(aux), aux.stride(0) if aux is not None else 0, epi_c, relu, P(part)]
    if plan is not None:
        args.append(plan)
    call(lib, entry, *args)
    if epi == 3:            # the slab's rows summed: test_psw_epilogues_and_colsums (rtol 1e-5, atol 1e-3)
        refs["colsum_part"] = (("colsum", ref.sum(0)), 1e-3, 1e-5)
    return refs


PSW_CASES = [dict(M=M, N=N, K=K, epi=0) for M, N, K in GEMM_MNK] + [
    dict(M=129, N=300, K=76, epi=1), dict(M=129, N=100, K=300, epi=2), dict(M=129, N=512, K=300, epi=3),
    dict(M=1, N=100, K=76, epi=3), dict(M=129, N=512, K=512, epi=2)]


@case("hsg_gemm_f32_psw", *PSW_CASES)
def c_gemm_f32_psw(lib, mk, M, N, K, epi):
    return _psw(lib, mk, "hsg_gemm_f32_psw", M, N, K, epi)


@case("hsg_gemm_f32_psw_plan", *[dict(M=M, N=512, K=K, epi=e, plan=p) for M in (1, 129) for K in (300, 512)
                                 for e, p in ((0, 13), (3, 13), (1, 13), (0, 7))],
      dict(M=129, N=300, K=76, epi=2, plan=13), dict(M=129, N=100, K=76, epi=0, plan=0))
def c_gemm_f32_psw_plan(lib, mk, M, N, K, epi, plan):
    """plan 13 at N = 512: k_gemm13 (160 x 128 blocks; 192 x 128 with colsum_part)."""
    return _psw(lib, mk, "hsg_gemm_f32_psw_plan", M, N, K, epi, plan=plan)


@case("hsg_gemm_bf16_psw", *PSW_CASES)
def c_gemm_bf16_psw(lib, mk, M, N, K, epi):
    return _psw(lib, mk, "hsg_gemm_bf16_psw", M, N, K, epi, bf16=True)


# ------------------------------------------------------------------------------------
# the bf16 GEMM mode's bf16 activations, the ELU-gate epilogues and the batched weight
# gradients
def _bf16_A(mk, A, K):
    """A bf16 A operand: pitch % 8 == 0, zeros in columns K .. ceil8(K) - 1 (the bf16-A
    contract, hsg.h), NaN in the rest of the pitch."""
    return mk.inp(A.bfloat16(), pitch=ceil_to(K, 8) + 8, zero_cols=ceil_to(K, 8) - K, plain_pitch=ceil_to(K, 8))


@case("hsg_gemm_bf16_psw_io", dict(M=129, N=512, K=300, io=2, epi=0), dict(M=129, N=300, K=512, io=1, epi=0),
      dict(M=129, N=512, K=300, io=7, epi=1), dict(M=1, N=100, K=76, io=3, epi=0),
      dict(M=129, N=64, K=300, io=1, epi=2), dict(M=1, N=512, K=300, io=7, epi=1))
def c_gemm_bf16_psw_io(lib, mk, M, N, K, io, epi):
    """io bits: 1 A bf16, 2 C bf16, 4 aux (the relu' mask) bf16; epi 0 store + bias + relu,
    1 relu' mask with colsum_part, 2 accumulate.  test_gpu_gemm.py::
    test_psw_bf16_mode_is_the_rounded_product: 1e-5 * max(1, |ref|_max) * max(1, sqrt(K)); a bf16
    C adds its RNE rounding (2^-9 |c|, hsg.h)."""
    A, W = r64(M, K), r64(N, K)
    planes, _, _, _ = _wsplit(lib, mk, W, N, K, 0)
    Ad = _bf16_A(mk, A, K) if io & 1 else mk.inp(A, pitch=ceil_to(K, 4) + 4, plain_pitch=ceil_to(K, 4))
    ref = A.bfloat16().double() @ W.bfloat16().double().t()
    bias = aux = part = init = None
    epi_c = relu = 0
    if epi == 0:
        bias, relu = r64(N), 1
        ref = torch.relu(ref + bias.double())
    elif epi == 1:
        auxv = r64(M, N)
        aux = mk.inp(auxv.bfloat16() if io & 4 else auxv, pitch=N + 8)
        epi_c, ref = 1, ref * (auxv.double() > 0)
    else:
        init, epi_c = r64(M, N), 2
        ref = ref + init.double()
    C = mk.out("C", M, N, torch.bfloat16 if io & 2 else torch.float32, pitch=N + 8, plain_pitch=N, init=init)
    tol = 1e-5 * max(1.0, ref.abs().max().item()) * max(1.0, K ** 0.5)
    refs = {"C": (ref, tol, 2.0 ** -8 if io & 2 else 0.0)}
    if epi == 1:
        part = mk.out("colsum_part", lib.hsg_gemm_psw_row_tiles(M, N, K, 1), N)
        refs["colsum_part"] = (("colsum", ref.sum(0)), 1e-3, 1e-5)
    if epi == 2:
        aux = C
    call(lib, "hsg_gemm_bf16_psw_io", M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0),
         P(mk.inp(bias)) if bias is not None else None, P(aux), aux.stride(0) if aux is not None else 0, epi_c, relu,
         P(part), io)
    return refs


def _elug(lib, mk, entry, M, a16=0, g16=0, x16=0, with_rho=1, bf16=0):
    """C = aux + A W1 (N = 300, K = 512), G = C * elu'(h) with elu(h) = x - origin, rho = the
    per-group per-head partials of G . h.  Tolerances: test_gpu_elug.py::test_psw_elug_matches_fp64
    (1e-4 * max(1, |C|_max) on C and G) and ::test_psw_elug_rho_partials (rho: the rounding of
    e = x - origin, delta <= 4 ulp(|x| + |origin|) + ulp(1), times |C| (|h| + 1), plus 1e-5 sum |G| (|h| + 1))."""
    N, K, D = 300, 512, 50
    bfm = bool(bf16 or a16)
    A, W, auxv, origin = r64(M, K), r64(N, K) / K ** 0.5, r64(M, N), r64(M, N)
    h = 2 * r64(M, N)
    h[::7] = 0.0
    x = torch.nn.functional.elu(h) + origin
    if x16:
        x = x.bfloat16()
    planes, _, _, _ = _wsplit(lib, mk, W, N, K, 0)
    a64, w64 = (A.bfloat16().double(), W.bfloat16().double()) if bfm else (A.double(), W.double())
    Cref = auxv.double() + a64 @ w64.t()
    e = x.double() - origin.double()
    Gref = torch.where(e > 0, Cref, Cref * (e + 1))
    ld = N + 8
    C = mk.out("C", M, N, pitch=N + 4)
    G = mk.out("G", M, N, torch.bfloat16 if g16 else torch.float32, pitch=ld, plain_pitch=ld)
    Ad = _bf16_A(mk, A, K) if a16 else mk.inp(A, pitch=K + 4)
    auxd, od = mk.inp(auxv, pitch=ld, plain_pitch=ld), mk.inp(origin, pitch=ld, plain_pitch=ld)
    xd = mk.inp(x, pitch=312, plain_pitch=312) if x16 else mk.inp(x, pitch=ld, plain_pitch=ld)
    scale = max(1.0, Cref.abs().max().item())
    refs = {"C": (Cref, 1e-4 * scale, 0.0), "G": (Gref, 1e-4 * scale, 2.0 ** -8 if g16 else 0.0)}
    rho = None
    if with_rho:
        gw = lib.hsg_gemm_psw_elug_rho_gw(M, N, K, D, int(bfm))
        ng = (N + gw - 1) // gw
        rho = mk.out("rho", M, ng * 3)
        hh = torch.where(e > 0, e, torch.log1p(e.clamp_min(-1 + 1e-300)))
        hh = torch.where(e <= -1, torch.zeros_like(hh), hh)

        def groups(t):
            out = torch.zeros(M, ng, 3, dtype=torch.float64)
            for g in range(ng):
                for c in range(gw * g, min(gw * (g + 1), N)):
                    out[:, g, c // D - (gw * g) // D] += t[:, c]
            return out.view(M, ng * 3)
        xf = x.double()
        delta = 4 * 2.0 ** -23 * (xf.abs() + origin.double().abs()) + 2.0 ** -23
        bound = groups(Cref.abs() * delta * (hh.abs() + 1)) + 1e-5 * groups(Gref.abs() * (hh.abs() + 1)) + 1e-12
        rref = groups(Gref * hh)

        def check_rho(got):
            err = (got.double() - rref).abs()
            assert bool((err <= bound).all()), ("rho", (err / bound).max().item())
        refs["rho"] = (check_rho, 0, 0)
    if entry == "hsg_gemm_f32_psw_elug":
        args = [M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0), P(auxd), P(xd), P(od), P(G), ld, bf16]
    elif entry == "hsg_gemm_psw_elug_rho":
        args = [M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0), P(auxd), P(xd), P(od), P(G), ld, P(rho), D,
                bf16]
    elif entry == "hsg_gemm_bf16_psw_elug_rho_a16":
        args = [M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0), P(auxd), P(xd), P(od), P(G), ld, P(rho), D,
                g16]
    else:
        args = [M, N, K, P(Ad), Ad.stride(0), P(planes), P(C), C.stride(0), P(auxd), P(xd), xd.stride(0), x16, P(od),
                P(G), ld, P(rho), D, g16]
    call(lib, entry, *args)
    return refs


@case("hsg_gemm_f32_psw_elug", dict(M=1, bf16=0), dict(M=129, bf16=0), dict(M=129, bf16=1))
def c_gemm_f32_psw_elug(lib, mk, M, bf16):
    return _elug(lib, mk, "hsg_gemm_f32_psw_elug", M, with_rho=0, bf16=bf16)


@case("hsg_gemm_psw_elug_rho", dict(M=1, bf16=0), dict(M=129, bf16=0), dict(M=129, bf16=1))
def c_gemm_psw_elug_rho(lib, mk, M, bf16):
    return _elug(lib, mk, "hsg_gemm_psw_elug_rho", M, bf16=bf16)


@case("hsg_gemm_bf16_psw_elug_rho_a16", dict(M=1, g16=0), dict(M=129, g16=1))
def c_gemm_bf16_psw_elug_rho_a16(lib, mk, M, g16):
    return _elug(lib, mk, "hsg_gemm_bf16_psw_elug_rho_a16", M, a16=1, g16=g16)


@case("hsg_gemm_bf16_psw_elug_rho_x16", dict(M=1, x16=1), dict(M=129, x16=1), dict(M=129, x16=0))
def c_gemm_bf16_psw_elug_rho_x16(lib, mk, M, x16):
    """x as bf16 rows of pitch 312 (hsg_gat_fwd_ws16's rows; the LayerNorm-style residual read
    asks nothing of its pad: NaN); x16 = 0 is the _a16 call."""
    return _elug(lib, mk, "hsg_gemm_bf16_psw_elug_rho_x16", M, a16=1, g16=1, x16=x16)


def _dw_slabs(lib, mk, K, splits, bf16, io=None):
    """One job pair at (300, 512): dW2 = A1^T B1 [300, 512] and dW1 = A2^T B2 [512, 300], ws_q
    [splits][M_q][N_q].  test_gpu_gemm.py::test_dw_slabs_pair: |err| < 2e-6 * sum_k |a_k b_k| per
    element of the slabs' sum."""
    shapes = [(300, 512), (512, 300)]
    i32, vp = ctypes.c_int, ctypes.c_void_p
    As, Bs, Ws, refs = [], [], [], {}
    for q, (M, N) in enumerate(shapes):
        A, B = r64(K, M), r64(K, N)
        ab = bool(io and io[q] & 1) or (bool(bf16) and io is None)
        bb = bool(io and io[q] & 2) or (bool(bf16) and io is None)
        a64 = A.bfloat16().double() if ab else A.double()
        b64 = B.bfloat16().double() if bb else B.double()
        if io is not None and not io[q] & 1:
            a64 = A.bfloat16().double()                     # the bf16 mode rounds an fp32 operand at fragment read
        if io is not None and not io[q] & 2:
            b64 = B.bfloat16().double()
        As.append(mk.inp(A.bfloat16() if io and io[q] & 1 else A, pitch=M + 8, plain_pitch=M))
        Bs.append(mk.inp(B.bfloat16() if io and io[q] & 2 else B, pitch=N + 8, plain_pitch=N))
        Ws.append(mk.out(f"ws{q}", splits, M * N))
        ref, unit = a64.t() @ b64, a64.abs().t() @ b64.abs()

        def check_sum(got, ref=ref, unit=unit, q=q):
            err = (got.double().sum(0).view(ref.shape) - ref).abs()
            assert bool((err <= 2e-6 * unit.clamp_min(1e-30)).all()), (q, (err / unit.clamp_min(1e-30)).max().item())
        refs[f"ws{q}"] = (check_sum, 0, 0)
    args = [2, _arr(i32, [m for m, _ in shapes]), _arr(i32, [n for _, n in shapes]), K, _arr(vp, [P(a) for a in As]),
            _arr(i32, [a.stride(0) for a in As]), _arr(vp, [P(b) for b in Bs]), _arr(i32, [b.stride(0) for b in Bs])]
    if io is not None:
        call(lib, "hsg_gemm_dw_slabs_io", *args, _arr(i32, io), splits, _arr(vp, [P(w) for w in Ws]))
    else:
        call(lib, "hsg_gemm_dw_slabs", *args, splits, bf16, _arr(vp, [P(w) for w in Ws]))
    return refs


@case("hsg_gemm_dw_slabs", dict(K=1, sp=1, bf16=0), dict(K=257, sp=3, bf16=0), dict(K=257, sp=3, bf16=1))
def c_gemm_dw_slabs(lib, mk, K, sp, bf16):
    return _dw_slabs(lib, mk, K, sp, bf16)


@case("hsg_gemm_dw_slabs_io", dict(K=1, sp=1, io0=3, io1=1), dict(K=257, sp=3, io0=3, io1=2),
      dict(K=257, sp=3, io0=1, io1=3))
def c_gemm_dw_slabs_io(lib, mk, K, sp, io0, io1):
    return _dw_slabs(lib, mk, K, sp, 1, io=[io0, io1])


# ------------------------------------------------------------------------------------
# LayerNorm / dropout row kernels and the narrow one-launch FFN.  n = 1 and 9: one
# (partial) row group of the persistent kernels plus a ragged one; d = 64 the scalar
# kernels, d = 300 the vector kernels (257..512 columns).
# Tolerances: test_gpu_ffn.py::test_ffn_train_matches_fp64_with_same_mask -- forward 2e-5
# absolute, gradients 1e-4 * max(1, |ref|_max).
SEED, OFFSET = 77, 5
LN_CASES = [dict(n=n, d=d, p=p) for n in (1, 9) for d in (64, 300) for p in (0.0, 0.1)]


def grad_tol(ref):
    return (1e-4 * max(1.0, ref.abs().max().item()), 0.0)


def _ln_ref(n, d, p, y, x, gamma, beta, dout=None):
    """fp64 forward (and backward) of out = LN(dropout(y) + x) with the kernels' keep mask."""
    from oracle import masks
    keep = torch.from_numpy(masks.ffn_keep(SEED, OFFSET, n, d, p)).double() if p > 0 else torch.ones(n, d).double()
    scale = masks.ffn_scale(p) if p > 0 else 1.0
    yl, xl, gl, bl = [t.double().clone().requires_grad_() for t in (y, x, gamma, beta)]
    s = yl * keep * scale + xl
    mean = s.mean(1)
    rstd = 1.0 / torch.sqrt(s.var(1, unbiased=False) + 1e-5)
    out = (s - mean[:, None]) * rstd[:, None] * gl + bl
    res = dict(out=out.detach(), mean=mean.detach(), rstd=rstd.detach())
    if dout is not None:
        (out * dout.double()).sum().backward()
        res.update(dx=xl.grad, dy=yl.grad, part=torch.cat([gl.grad, bl.grad, yl.grad.sum(0)]))
    return res


def _ln_fwd(lib, mk, entry, n, d, p, ybf=False, xbf=False, ldx=None):
    y, x, gamma, beta = r64(n, d), r64(n, d), 1 + 0.1 * r64(d), 0.1 * r64(d)
    if ybf:
        y = y.bfloat16()
    if xbf:
        x = x.bfloat16()
    r = _ln_ref(n, d, p, y, x, gamma, beta)
    out, mean, rstd = mk.out("out", n, d), mk.out("mean", 1, n), mk.out("rstd", 1, n)
    xd = mk.inp(x, pitch=ldx, plain_pitch=ceil_to(d, 8)) if xbf else mk.inp(x)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    args = [n, d, P(mk.inp(y)), P(xd)] + ([xd.stride(0)] if xbf else []) + [
        P(mk.inp(gamma)), P(mk.inp(beta)), 1e-5, p, P(seed), OFFSET, P(out), P(mean), P(rstd)]
    call(lib, entry, *args)
    one = lambda t: (t, 2e-5 * max(1.0, t.abs().max().item()), 0.0)
    return {"out": (r["out"], 2e-5, 0.0), "mean": one(r["mean"]), "rstd": one(r["rstd"])}


@case("hsg_ln_fwd", *LN_CASES)
def c_ln_fwd(lib, mk, n, d, p):
    return _ln_fwd(lib, mk, "hsg_ln_fwd", n, d, p)


@case("hsg_ln_fwd_y16", *[dict(n=n, p=p) for n in (1, 9) for p in (0.0, 0.1)])
def c_ln_fwd_y16(lib, mk, n, p):
    return _ln_fwd(lib, mk, "hsg_ln_fwd_y16", n, 300, p, ybf=True)


@case("hsg_ln_fwd_x16", *[dict(n=n, p=p, ldx=ldx) for n in (1, 9) for p, ldx in ((0.0, 304), (0.1, 320))])
def c_ln_fwd_x16(lib, mk, n, p, ldx):
    """x as bf16 rows of pitch 304 / 320: the header asks nothing of the pad columns of a
    LayerNorm residual, so they hold NaN."""
    return _ln_fwd(lib, mk, "hsg_ln_fwd_x16", n, 300, p, ybf=True, xbf=True, ldx=ldx)


def _ln_bwd(lib, mk, entry, n, d, p, ybf=False, xbf=False, ldx=None, ld_dy=None):
    y, x, gamma, beta, dout = r64(n, d), r64(n, d), 1 + 0.1 * r64(d), 0.1 * r64(d), r64(n, d)
    if ybf:
        y = y.bfloat16()
    if xbf:
        x = x.bfloat16()
    r = _ln_ref(n, d, p, y, x, gamma, beta, dout)
    nb = lib.hsg_ln_bwd_blocks(n)
    dx, part = mk.out("dx", n, d), mk.out("part", nb, 3 * d)
    if ld_dy:
        # hsg.h: zeros in columns d .. ceil8(d) - 1 of the bf16 dy rows; the rest of the pitch untouched
        dy = mk.out("dy", n, d, torch.bfloat16, pitch=ld_dy, plain_pitch=ld_dy, pad=("zero", ceil_to(d, 8) - d))
    else:
        dy = mk.out("dy", n, d)
    xd = mk.inp(x, pitch=ldx, plain_pitch=ceil_to(d, 8)) if xbf else mk.inp(x)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    args = [n, d, P(mk.inp(dout)), P(mk.inp(y))] + ([int(ybf)] if entry == "hsg_ln_bwd_dy16" else []) + [P(xd)] + (
        [xd.stride(0)] if xbf else []) + [P(mk.inp(gamma)), P(mk.inp(r["mean"].float())), P(mk.inp(r["rstd"].float())),
                                          p, P(seed), OFFSET, P(dy)] + ([ld_dy] if ld_dy else []) + [P(dx), P(part)]
    call(lib, entry, *args)
    dy_tol = grad_tol(r["dy"])
    if ld_dy:                                        # + the RNE rounding of the bf16 store (2^-9 |dy|; hsg.h)
        dy_tol = (dy_tol[0], 2.0 ** -8)
    return {"dx": (r["dx"], *grad_tol(r["dx"])), "dy": (r["dy"], *dy_tol),
            "part": (("colsum", r["part"]), *grad_tol(r["part"]))}


@case("hsg_ln_bwd", *LN_CASES)
def c_ln_bwd(lib, mk, n, d, p):
    return _ln_bwd(lib, mk, "hsg_ln_bwd", n, d, p)


@case("hsg_ln_bwd_dy16", *[dict(n=n, p=p, ybf=ybf, ld=ld) for n in (1, 9)
                           for p, ybf, ld in ((0.0, 0, 304), (0.1, 1, 320), (0.1, 0, 320))])
def c_ln_bwd_dy16(lib, mk, n, p, ybf, ld):
    return _ln_bwd(lib, mk, "hsg_ln_bwd_dy16", n, 300, p, ybf=bool(ybf), ld_dy=ld)


@case("hsg_ln_bwd_x16", *[dict(n=n, p=p, ldx=a, ld=b) for n in (1, 9)
                          for p, a, b in ((0.0, 304, 320), (0.1, 320, 304))])
def c_ln_bwd_x16(lib, mk, n, p, ldx, ld):
    return _ln_bwd(lib, mk, "hsg_ln_bwd_x16", n, 300, p, ybf=True, xbf=True, ldx=ldx, ld_dy=ld)


@case("hsg_ffn_colsums", dict(rh=1, rl=1, acc=0), dict(rh=3, rl=9, acc=1))
def c_ffn_colsums(lib, mk, rh, rl, acc):
    """db1 = column sums of hpart [rows_h][d_hid]; dgamma, dbeta, db2 of lnpart [rows_ln][3][d]
    (d = 300, d_hid = 100: neither a multiple of the 32-column blocks).
    test_gpu_gemm.py::test_slab_batch_sums_segments_in_one_launch: rtol 1e-5, atol 1e-4."""
    d, dh = 300, 100
    hpart, lnpart = r64(rh, dh), r64(rl, 3 * d)
    names = ("db1", "dgamma", "dbeta", "db2")
    inits = [r64(1, dh if k == "db1" else d) if acc else None for k in names]
    outs = [mk.out(k, 1, dh if k == "db1" else d, init=i) for k, i in zip(names, inits)]
    call(lib, "hsg_ffn_colsums", rh, dh, P(mk.inp(hpart)), P(outs[0]), rl, d, P(mk.inp(lnpart)), P(outs[1]), P(outs[2]),
         P(outs[3]), acc)
    ln = lnpart.double().view(rl, 3, d).sum(0)
    refs = [hpart.double().sum(0), ln[0], ln[1], ln[2]]
    return {k: ((r + i.double().view(-1)) if acc else r, 1e-4, 1e-5) for k, r, i in zip(names, refs, inits)}


def _ffn_small_ref(n, p):
    """fp64 restatement of the narrow FFN (d = 64, d_hid = 512) with the kernels' keep mask."""
    from oracle import masks
    d, dh = 64, 512
    v = dict(x=r64(n, d), w1=r64(dh, d) / d ** 0.5, b1=0.1 * r64(dh), w2=r64(d, dh) / dh ** 0.5, b2=0.1 * r64(d),
             gamma=1 + 0.1 * r64(d), beta=0.1 * r64(d), dout=r64(n, d), h_edge=r64(n, d))
    keep = torch.from_numpy(masks.ffn_keep(SEED, OFFSET, n, d, p)).double() if p > 0 else torch.ones(n, d).double()
    scale = masks.ffn_scale(p) if p > 0 else 1.0
    L = {k: t.double().clone().requires_grad_() for k, t in v.items()}
    pre = L["x"] @ L["w1"].t() + L["b1"]
    pre.retain_grad()
    H = torch.relu(pre)
    y = H @ L["w2"].t() + L["b2"]
    y.retain_grad()
    s = y * keep * scale + L["x"]
    mean = s.mean(1)
    rstd = 1.0 / torch.sqrt(s.var(1, unbiased=False) + 1e-5)
    out = (s - mean[:, None]) * rstd[:, None] * L["gamma"] + L["beta"]
    (out * L["dout"].detach()).sum().backward()
    r = dict(H=H.detach(), y=y.detach(), out=out.detach(), mean=mean.detach(), rstd=rstd.detach(), dy=y.grad,
             dH=pre.grad, dx=L["x"].grad, lnpart=torch.cat([L["gamma"].grad, L["beta"].grad, y.grad.sum(0)]),
             hpart=pre.grad.sum(0))
    he = v["h_edge"].double()
    G = r["dx"] * torch.where(he > 0, torch.ones_like(he), torch.exp(he))
    r.update(G=G, rho=(G * he).view(n, 8, 8).sum(-1))
    return v, r


FFN_SMALL = [dict(n=n, p=p) for n in (1, 16 * 2 + 5) for p in (0.0, 0.1)]


@case("hsg_ffn_small_fwd", *FFN_SMALL)
def c_ffn_small_fwd(lib, mk, n, p):
    v, r = _ffn_small_ref(n, p)
    d, dh = 64, 512
    H, y, out = mk.out("H", n, dh), mk.out("y", n, d), mk.out("out", n, d)
    mean, rstd = mk.out("mean", 1, n), mk.out("rstd", 1, n)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    call(lib, "hsg_ffn_small_fwd", n, d, dh, *[P(mk.inp(v[k])) for k in ("x", "w1", "b1", "w2", "b2", "gamma", "beta")],
         1e-5, p, P(seed), OFFSET, P(H), P(y), P(out), P(mean), P(rstd))
    one = lambda t: (t, 2e-5 * max(1.0, t.abs().max().item()), 0.0)
    # test_gpu_ffn.py::test_one_launch_narrow_ffn_matches_split_path: 2e-5 * max(1, |.|_max) on H, y, mean, rstd
    return {"out": (r["out"], 2e-5, 0.0), "H": one(r["H"]), "y": one(r["y"]), "mean": one(r["mean"]),
            "rstd": one(r["rstd"])}


def _ffn_small_bwd(lib, mk, n, p, gate):
    v, r = _ffn_small_ref(n, p)
    d, dh = 64, 512
    nb = lib.hsg_ffn_small_bwd_blocks(n)
    dy, dH, dx = mk.out("dy", n, d), mk.out("dH", n, dh), mk.out("dx", n, d)
    lnpart, hpart = mk.out("lnpart", nb, 3 * d), mk.out("hpart", nb, dh)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    args = [n, d, dh, P(mk.inp(v["dout"])), P(mk.inp(v["x"])), P(mk.inp(r["H"].float())), P(mk.inp(r["y"].float())),
            P(mk.inp(v["w1"])), P(mk.inp(v["w2"])), P(mk.inp(v["gamma"])), P(mk.inp(r["mean"].float())),
            P(mk.inp(r["rstd"].float())), p, P(seed), OFFSET, P(dy), P(dH), P(dx), P(lnpart), P(hpart)]
    refs = {k: (r[k], *grad_tol(r[k])) for k in ("dy", "dH", "dx")}
    refs["lnpart"] = (("colsum", r["lnpart"]), *grad_tol(r["lnpart"]))
    refs["hpart"] = (("colsum", r["hpart"]), *grad_tol(r["hpart"]))
    if gate:
        G, rho = mk.out("G", n, d), mk.out("rho", n, 8)
        args += [P(mk.inp(v["h_edge"])), P(G), P(rho)]
        refs.update(G=(r["G"], *grad_tol(r["G"])), rho=(r["rho"], *grad_tol(r["rho"])))
    call(lib, "hsg_ffn_small_bwd_gate" if gate else "hsg_ffn_small_bwd", *args)
    return refs


@case("hsg_ffn_small_bwd", *FFN_SMALL)
def c_ffn_small_bwd(lib, mk, n, p):
    return _ffn_small_bwd(lib, mk, n, p, False)


@case("hsg_ffn_small_bwd_gate", *FFN_SMALL)
def c_ffn_small_bwd_gate(lib, mk, n, p):
    """... plus G = dx * elu'(h_edge) and the per-head rho (the gradient tolerance of
    test_gpu_ffn.py; the edge backward that consumes them: test_gpu_elug.py)."""
    return _ffn_small_bwd(lib, mk, n, p, True)


# ------------------------------------------------------------------------------------
# head projection with per-head dropout, its keep masks and the step prologue.  n = 1 and
# 33 (a full 32-row mask word plus one row); (in, H, D) = (300, 8, 8) the narrow VALU
# shape, (64, 6, 50) the wide one; p = 0 and 0.1.
# Tolerances: test_gpu_hproj.py::test_head_projection_matches_masked_reference -- Z 1e-4
# absolute, gradients 1e-4 * max(1, |ref|_max); the masks bit-exact against oracle/masks.py
# (test_gpu_dropout_masks.py).
HP_SHAPES = [dict(n=n, d_in=i, H=H, D=D, p=p) for n in (1, 33) for i, H, D in ((300, 8, 8), (64, 6, 50))
             for p in (0.0, 0.1)]


def _mask_ref(n, d_in, H, p, offset=OFFSET):
    """(keep bool [H, n, in], the words [H * NWI, LDC] with the rows past n set, their
    defined-bit mask): the kernels must not depend on the bits of rows that do not exist."""
    from oracle import masks
    keep = masks.hproj_keep(SEED, offset, n, d_in, H, p)
    words = torch.from_numpy(masks.pack_hproj_bits(keep).copy())
    nwi = (n + 31) // 32
    defined = torch.zeros(nwi, dtype=torch.int64)
    for i in range(n):
        defined[i // 32] |= 1 << (i % 32)
    defined = defined.view(1, nwi, 1).expand(H, nwi, words.shape[-1]).reshape(H * nwi, -1).clone()
    defined[:, d_in:] = 0                            # LDC - in pad columns: written, no documented value
    words = words.reshape(H * nwi, -1)
    hostile = ((words.long() & 0xFFFFFFFF) | (~defined & 0xFFFFFFFF))
    hostile = torch.where(hostile >= 2 ** 31, hostile - 2 ** 32, hostile).to(torch.int32)
    return torch.from_numpy(keep), words, hostile, defined


def _bits_check(words, defined):
    def check(got):
        a = got.long().reshape(words.shape) & defined
        b = words.long() & defined
        bad = (a != b).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} mask words differ from oracle.masks, first at {bad[0].tolist()}"
    return check


def _mask_out(lib, mk, name, n, d_in, H, p, offset=OFFSET):
    _, words, _, defined = _mask_ref(n, d_in, H, p, offset)
    nw = lib.hsg_dropmask_words(n, d_in, H)
    assert nw == words.numel()
    bits = mk.out(name, words.shape[0], words.shape[1], torch.int32)
    return bits, _bits_check(words, defined)


@case("hsg_dropmask", *[dict(n=n, d_in=i, H=H, p=p) for n in (1, 33) for i, H in ((300, 8), (64, 6), (70, 3))
                        for p in (0.0, 0.1)])
def c_dropmask(lib, mk, n, d_in, H, p):
    """hsg_dropmask_words words, every one written (in = 70: LDC = 72, two pad columns per row of words)."""
    bits, chk = _mask_out(lib, mk, "bits", n, d_in, H, p)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    call(lib, "hsg_dropmask", n, d_in, H, p, P(seed), OFFSET, P(bits))
    return {"bits": (chk, 0, 0)}


MASK_JOBS = [(33, 300, 8, 0.1, 3), (1, 64, 6, 0.1, 5), (33, 70, 3, 0.0, 9)]


def _mask_jobs(lib, mk):
    i32, f32, u32, vp = ctypes.c_int, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p
    outs, refs = [], {}
    for q, (n, d_in, H, p, off) in enumerate(MASK_JOBS):
        b, chk = _mask_out(lib, mk, f"bits{q}", n, d_in, H, p, off)
        outs.append(b)
        refs[f"bits{q}"] = (chk, 0, 0)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    k = len(MASK_JOBS)
    args = [k, _arr(i32, [j[0] for j in MASK_JOBS]), _arr(i32, [j[1] for j in MASK_JOBS]),
            _arr(i32, [j[2] for j in MASK_JOBS]), _arr(f32, [j[3] for j in MASK_JOBS]), P(seed),
            _arr(u32, [j[4] for j in MASK_JOBS]), _arr(vp, [P(b) for b in outs])]
    return args, refs


def _wt(mk, refs):
    H, D, d_in = 8, 8, 300
    W = r64(H * D, d_in)
    Wt = mk.out("Wt", H * d_in, D)
    refs["Wt"] = (W.double().view(H, D, d_in).permute(0, 2, 1).reshape(H * d_in, D), 0.0, 0.0)
    return [H, D, d_in, P(mk.inp(W)), P(Wt)]


@case("hsg_dropmask_multi")
def c_dropmask_multi(lib, mk):
    args, refs = _mask_jobs(lib, mk)
    call(lib, "hsg_dropmask_multi", *args)
    return refs


@case("hsg_dropmask_multi_wt")
def c_dropmask_multi_wt(lib, mk):
    args, refs = _mask_jobs(lib, mk)
    call(lib, "hsg_dropmask_multi_wt", *args, *_wt(mk, refs))
    return refs


@case("hsg_step_prologue")
def c_step_prologue(lib, mk):
    """Masks, the narrow projection's weight transpose and two weights' limb planes in one launch."""
    args, refs = _mask_jobs(lib, mk)
    args += _wt(mk, refs)
    i32, vp = ctypes.c_int, ctypes.c_void_p
    specs = [(r64(512, 300), 512, 300, 0), (r64(512, 300), 300, 512, 1)]     # w_1 [N][K], w_2's transpose view
    Wd, planes = [], []
    for q, (W, N, K, trans) in enumerate(specs):
        Np, Kp = ceil_to(N, 128), ceil_to(K, 32)
        planes.append(mk.out(f"planes{q}", 3 * Np, Kp, torch.bfloat16))
        Wd.append(mk.inp(W, pitch=W.shape[1] + 3))
        Bm = (W.t() if trans else W).double()
        ref, rest = torch.zeros(3, Np, Kp, dtype=torch.float64), Bm.clone()
        for limb_i in range(3):
            limb = rest.float().bfloat16().double()
            ref[limb_i, :N, :K] = limb
            rest = rest - limb
        refs[f"planes{q}"] = (ref.view(3 * Np, Kp), 0.0, 0.0)
    args += [2, _arr(vp, [P(w) for w in Wd]), _arr(i32, [x[1] for x in specs]), _arr(i32, [x[2] for x in specs]),
             _arr(i32, [w.stride(0) for w in Wd]), _arr(i32, [x[3] for x in specs]), _arr(vp, [P(x) for x in planes])]
    call(lib, "hsg_step_prologue", *args)
    return refs


@case("hsg_seed_advance")
def c_seed_advance(lib, mk):
    seed = mk.out("seed", 1, 1, torch.int64, init=torch.tensor([[41]]))
    snap = mk.out("snap", 1, 1, torch.int64)
    call(lib, "hsg_seed_advance", P(seed), P(snap))
    r = torch.tensor([[42.0]], dtype=torch.float64)
    return {"seed": (r, 0, 0), "snap": (r, 0, 0)}


@case("hsg_hproj_wt", dict(H=8, D=8, d_in=300), dict(H=6, D=50, d_in=64))
def c_hproj_wt(lib, mk, H, D, d_in):
    W = r64(H * D, d_in)
    Wt = mk.out("Wt", H * d_in, D)
    call(lib, "hsg_hproj_wt", H, D, d_in, P(mk.inp(W)), P(Wt))
    return {"Wt": (W.double().view(H, D, d_in).permute(0, 2, 1).reshape(H * d_in, D), 0.0, 0.0)}


def _hp(n, d_in, H, D, p):
    keep, _, hostile, _ = _mask_ref(n, d_in, H, p)
    from oracle import masks
    X, W, a1 = r64(n, d_in), r64(H * D, d_in) / d_in ** 0.5, r64(H, D)
    dZ = r64(n, H * D)
    s = masks.hproj_scale(p)
    Xl, Wl = X.double().requires_grad_(), W.double().requires_grad_()
    Z = torch.einsum("kic,kdc->ikd", keep.double() * Xl.unsqueeze(0) * s, Wl.view(H, D, d_in)).reshape(n, H * D)
    (Z * dZ.double()).sum().backward()
    sigma = (Z.detach().view(n, H, D) * a1.double()).sum(-1)
    return dict(X=X, W=W, a1=a1, dZ=dZ, bits=hostile, Z=Z.detach(), sigma=sigma, dX=Xl.grad, dW=Wl.grad, s=s)


def _hproj_fwd(lib, mk, entry, n, d_in, H, D, p):
    v = _hp(n, d_in, H, D, p)
    HD = H * D
    Z = mk.out("Z", n, HD, pitch=HD + 4)
    Xd = mk.inp(v["X"], pitch=d_in + 4)
    bits = mk.ints(v["bits"])
    refs = {"Z": (v["Z"], 1e-4, 0.0)}
    if entry == "hsg_hproj_fwd_t8":
        Wt = mk.inp(v["W"].view(H, D, d_in).permute(0, 2, 1).reshape(H * d_in, D).contiguous())
        args = [n, d_in, H, P(Xd), Xd.stride(0), P(Wt), P(bits), p, P(Z), Z.stride(0)]
    else:
        args = [n, d_in, H, D, P(Xd), Xd.stride(0), P(mk.inp(v["W"])), P(bits), p, P(Z), Z.stride(0)]
    if entry != "hsg_hproj_fwd":
        sigma = mk.out("sigma", n, H)
        args += [P(mk.inp(v["a1"])), P(sigma)]
        refs["sigma"] = (v["sigma"], 1e-4 * max(1.0, v["sigma"].abs().max().item()), 0.0)
    call(lib, entry, *args)
    return refs


@case("hsg_hproj_fwd", *HP_SHAPES)
def c_hproj_fwd(lib, mk, n, d_in, H, D, p):
    return _hproj_fwd(lib, mk, "hsg_hproj_fwd", n, d_in, H, D, p)


@case("hsg_hproj_fwd_logits", *HP_SHAPES)
def c_hproj_fwd_logits(lib, mk, n, d_in, H, D, p):
    assert lib.hsg_hproj_fwd_logits_supported(H, D)
    return _hproj_fwd(lib, mk, "hsg_hproj_fwd_logits", n, d_in, H, D, p)


@case("hsg_hproj_fwd_t8", *[c for c in HP_SHAPES if c["D"] == 8])
def c_hproj_fwd_t8(lib, mk, n, d_in, H, D, p):
    assert lib.hsg_hproj_fwd_t8_supported(d_in, H, D)
    return _hproj_fwd(lib, mk, "hsg_hproj_fwd_t8", n, d_in, H, D, p)


@case("hsg_hproj_dx", *[dict(c, acc=a) for c, a in zip(HP_SHAPES, (0, 1) * 4)])
def c_hproj_dx(lib, mk, n, d_in, H, D, p, acc):
    v = _hp(n, d_in, H, D, p)
    init = r64(n, d_in) if acc else None
    dX = mk.out("dX", n, d_in, pitch=d_in + 4, init=init)
    dZ = mk.inp(v["dZ"], pitch=H * D + 4)
    call(lib, "hsg_hproj_dx", n, d_in, H, D, P(dZ), dZ.stride(0), P(mk.inp(v["W"])), P(mk.ints(v["bits"])), p, P(dX),
         dX.stride(0), acc)
    ref = v["dX"] + (init.double() if acc else 0)
    return {"dX": (ref, *grad_tol(v["dX"]))}


@case("hsg_hproj_dw", *[dict(c, mode=m) for c, m in zip(HP_SHAPES, (0, 1, 2, 0, 1, 2, 0, 1))])
def c_hproj_dw(lib, mk, n, d_in, H, D, p, mode):
    """mode 0: dW == NULL, only the hsg_hproj_dw_chunks slabs [H*D][in] (unscaled); 1: dW
    written; 2: dW accumulated into."""
    v = _hp(n, d_in, H, D, p)
    HD = H * D
    chunks = lib.hsg_hproj_dw_chunks(n, d_in, H, D)
    part = mk.out("part", chunks, HD * d_in)
    init = r64(HD, d_in) if mode == 2 else None
    dW = mk.out("dW", HD, d_in, init=init) if mode else None
    dZ, Xd = mk.inp(v["dZ"], pitch=HD + 4), mk.inp(v["X"], pitch=d_in + 4)
    call(lib, "hsg_hproj_dw", n, d_in, H, D, P(dZ), dZ.stride(0), P(Xd), Xd.stride(0), P(mk.ints(v["bits"])), p,
         P(part), P(dW), int(mode == 2))
    refs = {"part": (("colsum", (v["dW"] / v["s"]).reshape(-1)), *grad_tol(v["dW"]))}
    if mode:
        refs["dW"] = (v["dW"] + (init.double() if mode == 2 else 0), *grad_tol(v["dW"]))
    return refs


@case("hsg_hproj_bwd", *[dict(c, acc=a) for c, a in zip(HP_SHAPES, (1, 0) * 4)])
def c_hproj_bwd(lib, mk, n, d_in, H, D, p, acc):
    v = _hp(n, d_in, H, D, p)
    HD = H * D
    chunks = lib.hsg_hproj_dw_chunks(n, d_in, H, D)
    part = mk.out("part", chunks, HD * d_in)
    init = r64(n, d_in) if acc else None
    dX = mk.out("dX", n, d_in, pitch=d_in + 4, init=init)
    dZ, Xd = mk.inp(v["dZ"], pitch=HD + 4), mk.inp(v["X"], pitch=d_in + 4)
    call(lib, "hsg_hproj_bwd", n, d_in, H, D, P(dZ), dZ.stride(0), P(mk.inp(v["W"])), P(Xd), Xd.stride(0),
         P(mk.ints(v["bits"])), p, P(dX), dX.stride(0), acc, P(part))
    return {"dX": (v["dX"] + (init.double() if acc else 0), *grad_tol(v["dX"])),
            "part": (("colsum", (v["dW"] / v["s"]).reshape(-1)), *grad_tol(v["dW"]))}


# ------------------------------------------------------------------------------------
# sentence CNN encoder: n = 5 sentences of lengths {0, 1, 6, L, 3}, L = 20; Y and dY of
# pitch 1350 + 2.  Tolerances: test_gpu_encoder.py -- outputs 5e-5 absolute, gradients
# 1e-4 relative to the largest entry.
CNN_LENS, CNN_L, CNN_D = [0, 1, 6, 20, 3], 20, 300
HEIGHTS = (2, 3, 4, 5, 6, 7)


def _cnn_layout():
    rowoff = np.concatenate([[0], np.cumsum([g + 1 for g in CNN_LENS])])
    return torch.tensor(rowoff, dtype=torch.int32), int(rowoff[-1])


@case("hsg_cnn_gather")
def c_cnn_gather(lib, mk):
    n, L, D, V = len(CNN_LENS), CNN_L, CNN_D, 40
    rowoff, rows = _cnn_layout()
    ids = torch.zeros(n, L, dtype=torch.int64)
    for s_, g in enumerate(CNN_LENS):
        ids[s_, :g] = torch.randint(1, V, (g,))
    embed, pos = r64(V, D), r64(L + 1, D)
    X = mk.out("X", rows, D)
    call(lib, "hsg_cnn_gather", n, L, D, P(mk.ints(ids)), P(mk.inp(embed)), P(mk.inp(pos)), P(mk.ints(rowoff)), rows,
         P(X))
    ref = torch.zeros(rows, D, dtype=torch.float64)
    for s_, g in enumerate(CNN_LENS):
        for t in range(g):
            ref[rowoff[s_] + t] = embed[ids[s_, t]].double() + pos[t + 1].double()
        ref[rowoff[s_] + g] = embed[0].double() + pos[0].double()
    return {"X": (ref, 5e-5, 0.0)}


def _cnn_pool_ref(Y, bias):
    """feat / arg in fp64: windows t = 0 .. L - h over the sentence padded to L, every
    position past the sentence reading its one pad row."""
    n, L = len(CNN_LENS), CNN_L
    rowoff, _ = _cnn_layout()
    feat, arg = torch.zeros(n, 300, dtype=torch.float64), torch.zeros(n, 300, dtype=torch.int32)
    tap0 = 0
    for g_, h in enumerate(HEIGHTS):
        for s_, ln in enumerate(CNN_LENS):
            rows_ = torch.tensor([[int(rowoff[s_]) + min(t + i, ln) for i in range(h)] for t in range(L - h + 1)])
            acc = bias[g_].double().unsqueeze(0).expand(L - h + 1, 50).clone()
            for i in range(h):
                acc += Y[rows_[:, i], (tap0 + i) * 50:(tap0 + i + 1) * 50].double()
            mx, am = acc.max(0)
            # the first t of the max (CPU max_pool1d order)
            first = (acc == mx.unsqueeze(0)).int().argmax(0)
            feat[s_, g_ * 50:(g_ + 1) * 50] = torch.relu(mx)
            arg[s_, g_ * 50:(g_ + 1) * 50] = first.int()
        tap0 += h
    return feat, arg


@case("hsg_cnn_pool")
def c_cnn_pool(lib, mk):
    n, L = len(CNN_LENS), CNN_L
    rowoff, rows = _cnn_layout()
    Y, bias = r64(rows, 1350), [0.1 * r64(50) for _ in HEIGHTS]
    fref, aref = _cnn_pool_ref(Y, bias)
    feat, arg = mk.out("feat", n, 300), mk.out("arg", n, 300, torch.int32)
    Yd = mk.inp(Y, pitch=1352)
    bd = [mk.inp(b) for b in bias]
    call(lib, "hsg_cnn_pool", n, L, P(mk.ints(rowoff)), P(Yd), Yd.stride(0), _arr(ctypes.c_void_p, [P(b) for b in bd]),
         P(feat), P(arg))
    return {"feat": (fref, 5e-5, 0.0), "arg": (aref.double(), 0.0, 0.0)}


@case("hsg_cnn_pool_bwd")
def c_cnn_pool_bwd(lib, mk):
    n, L = len(CNN_LENS), CNN_L
    rowoff, rows = _cnn_layout()
    Y, bias = r64(rows, 1350), [0.1 * r64(50) for _ in HEIGHTS]
    fref, aref = _cnn_pool_ref(Y, bias)
    dfeat = r64(n, 300)
    dY = mk.out("dY", rows, 1350, pitch=1352, init=torch.zeros(rows, 1350))     # zero-filled by the caller
    call(lib, "hsg_cnn_pool_bwd", n, P(mk.ints(rowoff)), P(mk.inp(fref.float())), P(mk.ints(aref)), P(mk.inp(dfeat)),
         P(dY), dY.stride(0))
    ref = torch.zeros(rows, 1350, dtype=torch.float64)
    tap0 = 0
    for g_, h in enumerate(HEIGHTS):
        for s_, ln in enumerate(CNN_LENS):
            for c in range(50):
                col = g_ * 50 + c
                if fref[s_, col] > 0:
                    for i in range(h):
                        row = int(rowoff[s_]) + min(int(aref[s_, col]) + i, ln)
                        ref[row, (tap0 + i) * 50 + c] += dfeat[s_, col].double()
        tap0 += h
    return {"dY": (ref, 1e-4 * max(1.0, ref.abs().max().item()), 0.0)}


# ------------------------------------------------------------------------------------
# sentence LSTM: documents of lengths [1, 0, 3], one or two directions, every pitch wider
# than its columns.  Tolerance: test_gpu_lstm.py -- at most 4 x the error of the same
# recurrence in fp32 on the CPU against fp64, forward outputs never more than 1e-4; the
# fp64 restatement's h is checked against torch's fp64 nn.LSTM first.
LSTM_LENS, HID = [1, 0, 3], 128


def _lstm_ref(ndir, p, dtype):
    """Manual recurrence in `dtype` from pre = x W_ih^T + b: h, gates, c, y and dgates."""
    from oracle import masks
    torch.manual_seed(99)
    n, inp = sum(LSTM_LENS), 8
    lstm = torch.nn.LSTM(inp, HID, 1, batch_first=True, bidirectional=ndir == 2).double()
    x, dh_out = torch.randn(n, inp).double(), torch.randn(n, ndir * HID)
    sfx = ["", "_reverse"][:ndir]
    wih = torch.cat([getattr(lstm, "weight_ih_l0" + s_) for s_ in sfx]).detach()
    whh = torch.stack([getattr(lstm, "weight_hh_l0" + s_) for s_ in sfx]).detach()
    bias = torch.cat([getattr(lstm, "bias_ih_l0" + s_) + getattr(lstm, "bias_hh_l0" + s_) for s_ in sfx]).detach()
    pre32 = (x @ wih.t() + bias).float()                  # the kernel's input: the projection rounded to fp32
    pre = pre32.to(dtype).requires_grad_()
    w = whh.float().to(dtype)
    h = [[None] * ndir for _ in range(n)]
    gates, cs = [[None] * ndir for _ in range(n)], [[None] * ndir for _ in range(n)]
    off = 0
    for g in LSTM_LENS:
        for d in range(ndir):
            hp, cp = torch.zeros(HID, dtype=dtype), torch.zeros(HID, dtype=dtype)
            for t in (range(g) if d == 0 else range(g - 1, -1, -1)):
                a = pre[off + t, d * 4 * HID:(d + 1) * 4 * HID] + w[d] @ hp
                i_, f_, g_, o_ = a.view(4, HID)
                i_, f_, g_, o_ = torch.sigmoid(i_), torch.sigmoid(f_), torch.tanh(g_), torch.sigmoid(o_)
                cp = f_ * cp + i_ * g_
                hp = o_ * torch.tanh(cp)
                h[off + t][d], cs[off + t][d], gates[off + t][d] = hp, cp, torch.cat([i_, f_, g_, o_])
        off += g
    H = torch.stack([torch.cat(r) for r in h])
    keep = torch.from_numpy(masks.ffn_keep(SEED, OFFSET, n, ndir * HID, p)).to(dtype) if p > 0 else None
    y = H * keep * masks.ffn_scale(p) if p > 0 else H
    (y * dh_out.to(dtype)).sum().backward()
    res = dict(h=H.detach(), gates=torch.stack([torch.cat(r) for r in gates]).detach(),
               c=torch.stack([torch.cat(r) for r in cs]).detach(), y=y.detach(), dgates=pre.grad)
    if dtype == torch.float64:                            # the restatement is torch's nn.LSTM
        ref, o2 = [], 0
        for g in LSTM_LENS:
            if g:
                ref.append(lstm(x[o2:o2 + g].unsqueeze(0))[0][0].detach())
            o2 += g
        # (nn.LSTM ran on the unrounded projection: the fp32 rounding of pre moves h by ~1e-7)
        assert (torch.cat(ref) - res["h"]).abs().max().item() < 1e-5
    return dict(pre=pre32, whh=whh.float(), dh_out=dh_out), res


def _lstm_tol(r64_, r32, k, forward):
    yard = (r32[k].double() - r64_[k]).abs().max().item()
    return (min(4 * yard, 1e-4) if forward else 4 * yard, 0.0)


LSTM_CASES = [dict(ndir=nd, p=p) for nd in (1, 2) for p in (0.0, 0.1)]


@case("hsg_lstm_fwd", *LSTM_CASES)
def c_lstm_fwd(lib, mk, ndir, p):
    v, r = _lstm_ref(ndir, p, torch.float64)
    _, r32 = _lstm_ref(ndir, p, torch.float32)
    n, W = sum(LSTM_LENS), ndir * HID
    doc_off = torch.tensor(np.concatenate([[0], np.cumsum(LSTM_LENS)]), dtype=torch.int32)
    h = mk.out("h", n, W, pitch=W + 4)
    gates, c = mk.out("gates", n, 4 * W), mk.out("c", n, W)
    y = mk.out("y", n, W, pitch=W + 8) if p > 0 else None
    pre = mk.inp(v["pre"], pitch=4 * W + 4)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    call(lib, "hsg_lstm_fwd", len(LSTM_LENS), n, HID, ndir, P(mk.ints(doc_off)), P(pre), pre.stride(0),
         P(mk.inp(v["whh"].reshape(ndir * 4 * HID, HID))), P(h), h.stride(0), P(gates), P(c), p,
         P(seed) if p > 0 else None, OFFSET, P(y), y.stride(0) if p > 0 else 0)
    return {k: (r[k], *_lstm_tol(r, r32, k, True)) for k in ("h", "gates", "c") + (("y",) if p > 0 else ())}


@case("hsg_lstm_bwd", *LSTM_CASES)
def c_lstm_bwd(lib, mk, ndir, p):
    v, r = _lstm_ref(ndir, p, torch.float64)
    _, r32 = _lstm_ref(ndir, p, torch.float32)
    n, W = sum(LSTM_LENS), ndir * HID
    doc_off = torch.tensor(np.concatenate([[0], np.cumsum(LSTM_LENS)]), dtype=torch.int32)
    dgates = mk.out("dgates", n, 4 * W)
    dh = mk.inp(v["dh_out"], pitch=W + 4)
    seed = mk.ints(torch.tensor([SEED], dtype=torch.int64))
    call(lib, "hsg_lstm_bwd", len(LSTM_LENS), n, HID, ndir, P(mk.ints(doc_off)), P(dh), dh.stride(0),
         P(mk.inp(r["gates"].float())), P(mk.inp(r["c"].float())), P(mk.inp(v["whh"].reshape(ndir * 4 * HID, HID))), p,
         P(seed) if p > 0 else None, OFFSET, P(dgates))
    return {"dgates": (r["dgates"], *_lstm_tol(r, r32, "dgates", False))}


# ------------------------------------------------------------------------------------
# relation build: bit-exact against oracle.fused.typed_relation (test_gpu_relbuild.py)
@case("hsg_rel_build", dict(kind="W2S"), dict(kind="S2W"))
def c_rel_build(lib, mk, kind):
    """11 nodes, 40 edges; every output sized by the upper bounds n and E, the workspace
    exactly hsg_rel_build_workspace_bytes; the valid prefixes (counts) are the documented extent."""
    from test_gpu_relbuild import expected
    rng = np.random.default_rng(11)
    n, E = 11, 40
    unit = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 0], np.float32)
    src, dst = rng.integers(0, n, size=E), rng.integers(0, n, size=E)
    tffrac = rng.integers(0, 10, size=E)
    edtype = rng.choice(np.array([0.0, 1.0], np.float32), size=E, p=[0.8, 0.2])
    exp = expected(kind, src, dst, unit, tffrac, edtype)
    n_src, n_dst, n_typed = len(exp["src_nodes"]), len(exp["dst_nodes"]), len(exp["src"])
    assert n_typed > 0
    su, du = (0.0, 1.0) if kind == "W2S" else (1.0, 0.0)
    pre = lambda k, m: torch.arange(m) < k
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    spec = [("counts", 5, i32, 5), ("indptr", n + 1, i32, n_dst + 1), ("src", E, i32, n_typed), ("tf", E, u8, n_typed),
            ("eid", E, i64, n_typed), ("phantom", n, i32, n_dst), ("cindptr", n + 1, i32, n_src + 1),
            ("cdst", E, i32, n_typed), ("cperm", E, i32, n_typed), ("src_nodes", n, i64, n_src),
            ("dst_nodes", n, i64, n_dst)]
    # (past the valid prefixes the header promises nothing -- indptr, for one, is scanned over all n nodes)
    o = {k: mk.out(k, 1, m, dt, mask=pre(valid, m).view(1, m)) for k, m, dt, valid in spec}
    o["counts"].zero_()                                  # the caller zeroes the counters (relation.build_relation)
    wsb = lib.hsg_rel_build_workspace_bytes(n, E)
    assert wsb > 0
    ws = mk.scratch("ws", wsb, u8)
    t = lambda a, dt: mk.ints(torch.as_tensor(np.asarray(a), dtype=dt))
    call(lib, "hsg_rel_build", su, du, n, E, P(t(src, i64)), P(t(dst, i64)), P(t(unit, torch.float32)),
         P(t(tffrac, i64)), P(t(edtype, torch.float32)), *[P(o[k]) for k, *_ in spec], P(ws), wsb)
    refs = {}
    for k, m, dt, valid in spec[1:]:
        full = torch.zeros(1, m, dtype=torch.float64)
        full[0, :valid] = torch.from_numpy(np.asarray(exp[k]).astype(np.float64))
        refs[k] = (full, 0.0, 0.0)
    refs["counts"] = (torch.tensor([[n_src, n_dst, n_typed, 0, 0]], dtype=torch.float64), 0.0, 0.0)
    return refs


@case("hsg_rel_work", dict(which="indptr"), dict(which="cindptr"))
def c_rel_work(lib, mk, which):
    """work of exactly 5 * max_items int32 at the header's lower bound max_items = n + 2 *
    indptr[n] / min_len + 1: the items, then the zeroed counters, 5 * count words in all."""
    reld = relation("long")[0]
    ip = reld.dev[which].cpu()
    n, min_len, mult = ip.numel() - 1, 8, 1
    E = int(ip[-1])
    max_items = n + 2 * E // min_len + 1
    deg = (ip[1:] - ip[:-1]).tolist()
    Pn = max(min_len, mult * -(-E // n))
    count_ref = sum(-(-d // Pn) if d > Pn else 1 for d in deg)
    assert count_ref > n                                  # some node is split
    mask = (torch.arange(5 * max_items) < 5 * count_ref).view(1, -1)
    work = mk.out("work", 1, 5 * max_items, torch.int32, mask=mask, rest="untouched")
    count = mk.out("count", 1, 1, torch.int32)
    call(lib, "hsg_rel_work", n, P(mk.ints(ip.to(torch.int32))), min_len, mult, P(work), max_items, P(count))

    def check_work(got):
        got = got.view(-1)
        items, counters = got[:4 * count_ref].view(count_ref, 4).tolist(), got[4 * count_ref:5 * count_ref]
        assert not counters.any(), "arrival counters not zero"
        i = 0
        for v, d in enumerate(deg):
            if d <= Pn:
                assert items[i][0] == v, (i, items[i])
                i += 1
                continue
            npc, pos, first = -(-d // Pn), int(ip[v]), i
            for _ in range(npc):
                code, beg, end, fi = items[i]
                assert code == -(v + 1) and beg == pos and fi == first, (i, items[i])
                assert end - beg in (d // npc, -(-d // npc)), (i, items[i])          # near-equal pieces
                pos, i = end, i + 1
            assert pos == int(ip[v + 1])
        assert i == count_ref
    return {"work": (check_work, 0, 0), "count": (torch.tensor([[float(count_ref)]], dtype=torch.float64), 0.0, 0.0)}


# ------------------------------------------------------------------------------------
# the shared body
@pytest.mark.parametrize("fn,kw", _all_cases())
def test_guard_bands(fn, kw):
    run_case(fn, kw)


@pytest.mark.parametrize("H,D", [(8, 8), (6, 50)])
@pytest.mark.parametrize("ld", range(4))
def test_dev_tile_forward_ws16(monkeypatch, H, D, ld):
    """k_gat_fwd_tile<..., O16> (the destination-tile forward, compiled into the dev library
    only: HSG_GAT_FWD_TILE=1, short segments) has the same whole-node bf16 epilogue as
    k_gat_fwd: the hsg_gat_fwd_ws16 case at every pitch, against libhsg_dev.so."""
    from helpers import skip_unless_dev
    skip_unless_dev(False)
    monkeypatch.setenv("HSG_GAT_FWD_TILE", "1")
    run_case(c_gat_fwd_ws16, dict(kind="short", H=H, D=D, ld=ld))


def run_case(fn, kw):
    from hetersumgraph_amd._lib import load
    lib = load()
    runs = []
    for guarded_mode in (True, False):
        torch.manual_seed(SEED)
        mk = Alloc(guarded_mode)
        refs = fn(lib, mk, **kw)
        torch.cuda.synchronize()
        runs.append((mk, refs))
    (g, refs), (p, _) = runs
    assert g.outs.keys() == p.outs.keys() and set(refs) <= set(g.outs)
    for name, o in g.outs.items():                    # 1. nothing outside the documented extent
        o["h"].assert_guards_intact(name)
    for i, (buf, snap) in enumerate(g.inputs):        #    ... and the const operands, guards and pad included
        assert torch.equal(_bits(buf), _bits(snap)), f"input {i} (or its guards) was written"
    for name, o in g.outs.items():
        if o["scratch"]:
            continue
        h = o["h"]
        h.assert_fully_written(o["mask"], name)       # 2. every documented element
        if o["rest"] == "untouched":                  #    ... and nothing past the documented extent
            out_of = (h._payload() != h.pattern) & ~o["mask"].to(DEV).view(h.rows, h.cols)
            assert not bool(out_of.any()), (f"{name}: {int(out_of.sum())} elements outside the documented extent "
                                            f"were written, first at {out_of.nonzero()[0].tolist()}")
        if isinstance(o["pad"], tuple):               # 3. pad columns untouched / zero
            h.assert_pad(o["pad"][0], name, zero_cols=o["pad"][1])
        else:
            h.assert_pad(o["pad"], name)
        if o["finite"]:
            h.assert_finite(o["mask"], name)          # 4. no NaN / Inf
        a, b = _bits(o["t"]), _bits(p.outs[name]["t"])
        if o["mask"] is not None:
            keep = o["mask"].to(a.device).view(a.shape)
            a, b = a[keep], b[keep]
        diff = (a != b).nonzero()                     # 5. placement independence, bitwise
        assert diff.numel() == 0, (f"{name}: {diff.shape[0]} elements differ between the guarded and the plain run, "
                                   f"first at {diff[0].tolist()}")
    for name, (ref, atol, rtol) in refs.items():      # 6. values, against the fp64 restatement
        if callable(ref):
            ref(g.outs[name]["t"].cpu())
            continue
        got = g.outs[name]["t"].double().cpu()
        if isinstance(ref, tuple) and ref[0] == "colsum":
            got, ref = got.sum(0), ref[1]
        ref = ref.reshape(got.shape)
        mask = g.outs[name]["mask"]
        err = (got - ref).abs() - (atol + rtol * ref.abs())
        if mask is not None:
            err = err[mask.view(err.shape)]
        assert err.numel() == 0 or err.max().item() <= 0, (name, (got - ref).abs().max().item(), atol, rtol)
