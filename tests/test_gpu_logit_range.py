"""Edge-softmax parity at large, negative and saturated attention logits.

Softmax is shift-invariant, so with logits within a few units of zero (what every other
fp64 comparison of an edge kernel draws) a kernel that drops the max subtraction, starts
the running maximum at 0 for a destination without phantoms, or botches a rescale by
exp(m_old - m_new) still computes the right answer.  Here every edge entry point of
include/hsg.h runs under the logit regimes of tests/edge_ref.py:

  unit     tau = g                         control: today's inputs at today's bound
  offset+  tau = 100 + g                   an unshifted exp overflows
  offset-  tau = -1.2e4 + 100 g            post-leaky about -120: an unshifted exp underflows, a
                                           maximum floored at 0 gives l = 0
  spread   tau rows -2e4 .. 150, + g       saturated softmax, every rescale factor exactly 0;
           ('asc' / 'desc': the long destination's rows sorted -- its maximum arrives in the
           last / the first batch or piece)
  ties     tau = 100, a1 = 0               all logits equal: h is the segment mean (closed form)

on the three guard-band relations (97 x 61; 'short', 'long', 'long_wl') at the head shapes
(8, 8) and (6, 50), by direct calls on plain tensors at the product dispatch, and through
``ops.gat_aggregate`` / ``ops.gat_heads_table`` with autograd.

Bound, per compared tensor: ref64 is the restatement in fp64, yard the max-abs error of the
SAME restatement run in torch fp32 on the CPU from the same fp32 inputs -- for a backward
entry point that means the (m, l), h, G, rho, dpre it is handed as well: these are the fp64
forward's, rounded, and an fp32 backward that recomputes alpha from a logit near 150 (ulp
1.5e-5) no longer agrees with such an h to better than that, so sum_e dpre_e of a destination
stops cancelling and shows in d tau (measured: 9e-5 for kernel and yardstick alike; an fp32
run that continues from its OWN forward hides it, 4e-6).  The kernel may err
by max(existing bound, 4 x yard) -- the existing bound being 2e-5 absolute for h / out / m,
2e-5 max(1, |ref|_max) for l and the gradients, plus 2^-8 |x| for bf16 rows, and 4 the factor
tests/test_gpu_lstm.py grants a kernel whose summation order differs from torch's.  (At a
logit near 150 one fp32 ulp of the logit is 1.5e-5: a fixed 2e-5 cannot be the bound there.)
In regime 'unit' 4 x yard <= existing bound is asserted too, so the control runs at today's
tolerance.  Every element is compared and must be finite; outputs start as NaN.
Each comparison prints ``entry regime name err yard``; the worst err / yard per entry point
and regime is printed at the end of the module (DESIGN.md section 4 records them).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import edge_ref as er
from edge_ref import N_DST, N_SRC
from helpers import skip_unless_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(8, 8), (6, 50)]
WORST = {}                                   # (entry, regime) -> (err / yard, tensor name)


def regime_cases(kind):
    rc = [(r, None) for r in er.REGIMES]
    return rc + ([("spread", "asc"), ("spread", "desc")] if kind != "short" else [])


def cases(kinds, shapes=SHAPES, **extra):
    return [pytest.param(k, H, D, r, o, *extra.values(), id="-".join(
        [k, f"{H}x{D}", r + ("-" + o if o else "")] + [f"{n}{x}" for n, x in extra.items()]))
        for k in kinds for H, D in shapes for r, o in regime_cases(k)]


@functools.lru_cache(maxsize=None)
def refs(kind, order, H, D, regime, g_bf16=False, om=1):
    """(device relation, arrays, inputs incl. what a kernel is handed from the fp64 run, fp64
    results, yardsticks) -- computed once per case and shared."""
    reld, *arrays = er.relation(kind, order)
    torch.manual_seed(er.SEED)
    v = er.draw(H, D, regime, dout=True)
    r64, handed = er.restate(arrays, v, H, D, torch.float64, g_bf16, om)
    v.update(handed)
    f = lambda *ks: {k: r64[k].float() for k in ks}
    Gd = {"G": handed["G16"].float() if g_bf16 else r64["G"].float()}
    # the yardsticks: the fp32 run from the inputs of the forward, and from those of each
    # backward entry point -- the (m, l), h, G, rho, dpre it is handed (module docstring)
    given = dict(fwd=None, dst=f("m", "l", "h"), dst_g=f("m", "l", "G"), src=f("m", "l", "G", "dpre"),
                 src_g={**f("m", "l", "rho"), **Gd})
    yard = {k: er.yardstick(r64, er.restate(arrays, v, H, D, torch.float32, g_bf16, om, given=g)[0])
            for k, g in given.items()}
    return reld, arrays, v, r64, yard


def compare(entry, regime, name, got, ref, yard, key=None, bf16=False):
    """got (device tensor) against ref (fp64) with the module's bound; key: the name the
    existing bound goes by (edge_ref.existing_bound)."""
    got = got.detach().double().cpu()
    ref = ref.reshape(got.shape)
    assert torch.isfinite(got).all(), f"{entry} [{regime}] {name}: {int((~torch.isfinite(got)).sum())} non-finite"
    existing = er.existing_bound(key or name, ref)
    diff = (got - ref).abs()
    err = diff.max().item() if diff.numel() else 0.0
    print(f"{entry} {regime} {name} err {err:.3g} yard {yard:.3g} existing {existing:.3g}")
    if yard > 0:
        w = WORST.get((entry, regime), (0.0, ""))
        if err / yard > w[0] and not bf16:
            WORST[(entry, regime)] = (err / yard, name)
    if regime == "unit":
        assert 4 * yard <= existing, f"{entry} {name}: the control's yardstick {yard} exceeds today's bound {existing}"
    tol = max(existing, 4 * yard) + ((2.0 ** -8) * ref.abs() if bf16 else 0.0)
    assert bool((diff <= tol).all()), (entry, regime, name, err, yard, existing)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\nworst err / yard per entry point and regime")
    for (entry, regime), (ratio, name) in sorted(WORST.items()):
        print(f"RATIO {entry} {regime} {ratio:.2f} {name}")


def lib_():
    from hetersumgraph_amd._lib import load
    return load()


def P(t):
    return None if t is None else t.data_ptr()


KEEP = []                                    # the operands of the launch in flight (P() takes bare addresses)


def call(name, *args):
    from hetersumgraph_amd._lib import check
    check(getattr(lib_(), name)(*args, torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()
    KEEP.clear()


def dv(t):
    """A CPU tensor on the device, alive until the next call() has completed."""
    KEEP.append(t.detach().to(DEV).contiguous())
    return KEEP[-1]


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def rid(regime, order):
    return regime + ("-" + order if order else "")


# ------------------------------------------------------------------------------------
# forward
@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("regime", er.REGIMES)
def test_attn_src_logits(H, D, regime):
    _, _, v, r, yard = refs("short", None, H, D, regime)
    sigma = nan(N_SRC, H)
    call("hsg_attn_src_logits", N_SRC, H, D, P(dv(v["Z"])), P(dv(v["a1"])), P(sigma))
    compare("hsg_attn_src_logits", regime, "sigma", sigma, r["sigma"], yard["fwd"]["sigma"])


def _fwd_checks(entry, kind, order, H, D, regime, h, out, m, l, x16=None):
    _, arrays, v, r, yard = refs(kind, order, H, D, regime)
    tag, yard = rid(regime, order), yard["fwd"]
    if h is not None:
        compare(entry, tag, "h", h, r["h"], yard["h"])
        compare(entry, tag, "out", out, r["x"], yard["x"])
        if regime == "ties":                 # alpha = 1 / (deg + c e^-100): the segment mean
            compare(entry, tag, "h_closed_form", h, er.ties_closed_form(arrays, v["Z"], H, D), yard["h"], key="h")
    if x16 is not None:
        compare(entry, tag, "x16", x16, r["x"], yard["x"], bf16=True)
    compare(entry, tag, "m", m, r["m_saved"], yard["m_saved"])
    compare(entry, tag, "l", l, r["l_saved"], yard["l_saved"])
    if regime == "offset-":                  # with phantoms: m = 0, h ~ 0, l ~ c; without: an ordinary softmax
        ph = torch.as_tensor(arrays[3])
        typed = torch.zeros(N_DST, dtype=torch.bool).index_fill(0, torch.as_tensor(arrays[1]).long(), True)
        with_c, without = typed & (ph > 0), typed & (ph == 0)
        assert with_c.any() and without.any()
        lc = l.cpu()
        assert (m.cpu()[with_c] == 0).all() and (lc[with_c] - ph[with_c].unsqueeze(1)).abs().max() < 1e-6
        assert (m.cpu()[without] < -100).all() and (lc[without] >= 1).all()
        if h is not None:
            hc = h.cpu()
            assert hc[with_c].abs().max() < 1e-30
            assert (hc[without].view(-1, H, D).abs().amax(-1) > 1e-3).all()


def _fwd(kind, order, H, D, regime, entry):
    reld, _, v, _, _ = refs(kind, order, H, D, regime)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    h, out, m, l = nan(N_DST, HD), nan(N_DST, HD), nan(N_DST, H), nan(N_DST, H)
    args = [relp, H, D, 0, 0.01, P(dv(v["Z"])), P(dv(v["sigma"])), P(dv(v["tau"])), P(dv(v["origin"])), P(h), P(out),
            P(m), P(l)]
    if entry == "hsg_gat_fwd_ws":
        nws = lib_().hsg_gat_fwd_ws_floats(relp, H, D)
        assert nws > 0
        ws = nan(nws)
        args.append(P(ws))
    call(entry, *args)
    _fwd_checks(entry, kind, order, H, D, regime, h, out, m, l)


@pytest.mark.parametrize("kind,H,D,regime,order", cases(("short", "long")))
def test_gat_fwd(kind, H, D, regime, order):
    """'short': one wave per destination, 'long': four, whose partial (m, l, h) merge."""
    _fwd(kind, order, H, D, regime, "hsg_gat_fwd")


@pytest.mark.parametrize("kind,H,D,regime,order", cases(("long_wl",)))
def test_gat_fwd_ws_inline_merge(kind, H, D, regime, order):
    """The CSR work list: the long destinations' pieces merged by the last arriving block."""
    _fwd(kind, order, H, D, regime, "hsg_gat_fwd_ws")


@pytest.mark.parametrize("kind,H,D,regime,order", cases(("long_wl",)))
def test_gat_fwd_ws_merge_launch(monkeypatch, kind, H, D, regime, order):
    """The pieces merged by the second launch, k_gat_fwd_merge (HSG_PIECE_INLINE=0: the dev
    library reads the switch, the product library merges in-kernel whatever it says)."""
    skip_unless_dev(False)
    monkeypatch.setenv("HSG_PIECE_INLINE", "0")
    _fwd(kind, order, H, D, regime, "hsg_gat_fwd_ws")


@pytest.mark.parametrize("kind,H,D,regime,order", cases(("short", "long", "long_wl")))
def test_gat_fwd_ws16(kind, H, D, regime, order):
    """x = elu(h) + origin as bf16 rows (pitch ceil64(H D) + 8: pad columns, which must be zero)."""
    reld, _, v, _, _ = refs(kind, order, H, D, regime)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    ld16 = (HD + 63) // 64 * 64 + 8
    nws = lib_().hsg_gat_fwd_ws_floats(relp, H, D)
    assert (nws > 0) == (kind == "long_wl")
    ws = nan(nws) if nws else None
    x16, m, l = nan(N_DST, ld16, dtype=torch.bfloat16), nan(N_DST, H), nan(N_DST, H)
    call("hsg_gat_fwd_ws16", relp, H, D, 0, 0.01, P(dv(v["Z"])), P(dv(v["sigma"])), P(dv(v["tau"])),
         P(dv(v["origin"])), None, None, P(m), P(l), P(ws), P(x16), ld16)
    assert (x16[:, HD:] == 0).all()
    _fwd_checks("hsg_gat_fwd_ws16", kind, order, H, D, regime, None, None, m, l, x16=x16[:, :HD])


# ------------------------------------------------------------------------------------
# backward: the kernels are handed the fp64 forward's (h, m, l) / G / dpre rounded to fp32
def _dst_checks(entry, tag, r, yard, G, dpre, dtp):
    if G is not None:
        compare(entry, tag, "G", G, r["G"], yard["G"])
    compare(entry, tag, "dpre", dpre, r["dpre"], yard["dpre"])
    compare(entry, tag, "dtau", dtp.sum(0), r["dtau"], yard["dtau"])


@pytest.mark.parametrize("kind,H,D,regime,order,om", cases(("short", "long"), om=1) + cases(("short", "long"), om=0))
def test_gat_bwd_dst(kind, H, D, regime, order, om):
    """om 1: G = dOut * elu'(h) (out = elu(h) + origin); om 0: no origin, G = dOut."""
    reld, _, v, r, yard = refs(kind, order, H, D, regime, om=om)
    relp, HD, E = ctypes.byref(reld.cstruct()), H * D, r["dpre"].shape[0]
    nb = lib_().hsg_gat_bwd_blocks(relp)
    G, dpre, dtp = nan(N_DST, HD), nan(E, H), nan(nb, 11 * H)
    call("hsg_gat_bwd_dst", relp, H, D, 0, om, 0.01, P(dv(v["Z"])), P(dv(v["sigma"])), P(dv(v["tau"])),
         P(dv(r["h"].float())), P(dv(r["m"].float())), P(dv(r["l"].float())), P(dv(v["dout"])), P(G), P(dpre), P(dtp))
    _dst_checks(f"hsg_gat_bwd_dst(om={om})", rid(regime, order), r, yard["dst"], G, dpre, dtp)


@pytest.mark.parametrize("kind,H,D,regime,order", cases(("short",), [(6, 50)]))
@pytest.mark.parametrize("entry", ["hsg_gat_bwd_dst_noh", "hsg_gat_bwd_dst_g"])
def test_gat_bwd_dst_noh_and_g(entry, kind, H, D, regime, order):
    """The forward without h (short segments, D > 16): elu'(h) from x - origin; and the
    variant that is handed G."""
    reld, _, v, r, yard = refs(kind, order, H, D, regime)
    relp, HD, E = ctypes.byref(reld.cstruct()), H * D, r["dpre"].shape[0]
    assert lib_().hsg_gat_bwd_dst_noh_supported(relp, H, D)
    nb = lib_().hsg_gat_bwd_blocks(relp)
    dpre, dtp = nan(E, H), nan(nb, 11 * H)
    head = [relp, H, D, 0, 0.01, P(dv(v["Z"])), P(dv(v["sigma"])), P(dv(v["tau"]))]
    ml = [P(dv(r["m"].float())), P(dv(r["l"].float()))]
    if entry == "hsg_gat_bwd_dst_noh":
        G = nan(N_DST, HD)
        call(entry, *head, P(dv(r["x"].float())), P(dv(v["origin"])), *ml, P(dv(v["dout"])), P(G), P(dpre), P(dtp))
    else:
        G = None
        call(entry, *head, *ml, P(dv(r["G"].float())), P(dpre), P(dtp))
    _dst_checks(entry, rid(regime, order), r, yard["dst" if G is not None else "dst_g"], G, dpre, dtp)


@pytest.mark.parametrize("kind,H,D,regime,order,full", cases(("short", "long"), full=1) + cases(("short", "long"), full=0))
def test_gat_bwd_src(kind, H, D, regime, order, full):
    """full: a1 folded into dZ, dsigma and the da1 partials written; else dZ alone."""
    reld, _, v, r, yard = refs(kind, order, H, D, regime)
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    nb = lib_().hsg_gat_bwd_src_blocks(relp)
    dZ = nan(N_SRC, HD)
    dsig, da1p = (nan(N_SRC, H), nan(nb, HD)) if full else (None, None)
    call("hsg_gat_bwd_src", relp, H, D, 0, 0.01, P(dv(v["sigma"])), P(dv(v["tau"])), P(dv(r["m"].float())),
         P(dv(r["l"].float())), P(dv(r["G"].float())), P(dv(r["dpre"].float())), P(dv(v["a1"])) if full else None,
         P(dv(v["Z"])) if full else None, P(dZ), P(dsig), P(da1p))
    entry, tag, yard = f"hsg_gat_bwd_src(full={full})", rid(regime, order), yard["src"]
    if not full:
        compare(entry, tag, "dZ", dZ, r["dZ0"], yard["dZ0"])
        return
    compare(entry, tag, "dZ", dZ, r["dZ"], yard["dZ"])
    compare(entry, tag, "dsigma", dsig, r["dsigma"], yard["dsigma"])
    compare(entry, tag, "da1", da1p.sum(0), r["da1"], yard["da1"])


def _src_g(entry, kind, order, H, D, regime, g_bf16=0, dsig=1):
    """The one-pass source side (recomputes alpha and dpre per edge from (m, l), G and rho):
    narrow heads with per-head rho, wide heads with the 64-column-group partials."""
    reld, _, v, r, yard = refs(kind, order, H, D, regime, g_bf16=bool(g_bf16))
    relp, HD = ctypes.byref(reld.cstruct()), H * D
    lib = lib_()
    assert lib.hsg_gat_bwd_src_g_supported(relp, H, D)
    wide = D >= 32
    nb = lib.hsg_gat_bwd_src_g_blocks(relp, H, D)
    rho = r["rho_groups"].reshape(N_DST, -1) if wide else r["rho"]
    groups = (HD + 63) // 64 if wide else 0
    dZ, dsigma = nan(N_SRC, HD), nan(N_SRC, H) if dsig else None
    da1p, dtp = nan(nb, HD), nan(nb, 11 * H)
    Gd = dv(v["G16"]) if g_bf16 else dv(r["G"].float())
    args = [relp, H, D, 0.01, P(dv(v["sigma"])), P(dv(v["tau"])), P(dv(r["m"].float())), P(dv(r["l"].float())),
            P(Gd)] + ([g_bf16] if entry != "hsg_gat_bwd_src_g" else []) + [
        P(dv(rho.float())), groups, P(dv(v["a1"])), P(dv(v["Z"])), P(dZ), P(dsigma), P(da1p), P(dtp)]
    if entry == "hsg_gat_bwd_src_g_ws":
        nws = lib.hsg_gat_bwd_src_g_ws_floats(relp, H, D)
        assert (nws > 0) == (kind == "long_wl" and wide)
        ws = nan(nws) if nws else None
        args.append(P(ws))
    call(entry, *args)
    name = entry + ("(bf16 G)" if g_bf16 else "") + ("(pieces)" if kind == "long_wl" else "")
    tag, yard = rid(regime, order), yard["src_g"]
    compare(name, tag, "dZ", dZ, r["dZ"], yard["dZ"])
    compare(name, tag, "da1", da1p.sum(0), r["da1"], yard["da1"])
    compare(name, tag, "dtau", dtp.sum(0), r["dtau"], yard["dtau"])
    if dsig:
        compare(name, tag, "dsigma", dsigma, r["dsigma"], yard["dsigma"])


SRCG = cases(("short",), [(8, 8)]) + cases(("long",), [(6, 50)])    # the narrow head-lane kernel, the wide one


@pytest.mark.parametrize("kind,H,D,regime,order", SRCG)
def test_gat_bwd_src_g(kind, H, D, regime, order):
    _src_g("hsg_gat_bwd_src_g", kind, order, H, D, regime)


@pytest.mark.parametrize("kind,H,D,regime,order,g_bf16,dsig", [pytest.param(*p.values, 0, 1, id=p.id) for p in SRCG] + cases(
    ("long",), [(6, 50)], g_bf16=1, dsig=0))
def test_gat_bwd_src_g_io(kind, H, D, regime, order, g_bf16, dsig):
    _src_g("hsg_gat_bwd_src_g_io", kind, order, H, D, regime, g_bf16, dsig)


@pytest.mark.parametrize("kind,H,D,regime,order,g_bf16,dsig", [pytest.param(*p.values, 0, 1, id=p.id) for p in SRCG] + cases(
    ("long_wl",), [(6, 50)], g_bf16=0, dsig=1) + cases(("long_wl",), [(6, 50)], g_bf16=1, dsig=0))
def test_gat_bwd_src_g_ws(kind, H, D, regime, order, g_bf16, dsig):
    """'long_wl': the CSC work list -- pieces of the long sources, summed in piece order by
    the second launch."""
    _src_g("hsg_gat_bwd_src_g_ws", kind, order, H, D, regime, g_bf16, dsig)


# ------------------------------------------------------------------------------------
# autograd level: the product dispatch of ops.py, and the dev variants the existing tests sweep
VARIANTS = {"default": {}, "lpn16": {"HSG_GAT_LPN": "16"}, "lpn32": {"HSG_GAT_LPN": "32"},
            "lpn64-nopf": {"HSG_GAT_LPN": "64", "HSG_GAT_FWD_PF": "0"}, "src-hl0": {"HSG_GAT_SRC_HL": "0"},
            **{f"rows{q}": {"HSG_GAT_ROWS": q} for q in ("-1", "1", "2", "3", "5", "8")}}


def variant_cases():
    out = []
    for name in VARIANTS:
        for k in (("short", "long", "long_wl") if name == "default" else ("short", "long")):
            for H, D in SHAPES:
                for r, o in regime_cases(k) if name == "default" else [(r, None) for r in er.REGIMES]:
                    out.append(pytest.param(name, k, H, D, r, o, id=f"{name}-{k}-{H}x{D}-{rid(r, o)}"))
    return out


def _oracle(arrays, v, H, D, dtype, per_edge):
    from oracle.fused import gat_aggregate_ref
    e_src, e_dst, tf, phantom = arrays
    tfl = torch.as_tensor(tf).long()
    tau = v["tau"][tfl] if per_edge else v["tau"]            # per-edge mode: tau_row[tf[e]] per edge
    rows = np.arange(len(e_src)) if per_edge else tf
    Z, a1, tau, org = (t.to(dtype).clone().requires_grad_() for t in (v["Z"], v["a1"], tau, v["origin"]))
    out = gat_aggregate_ref(e_src, e_dst, rows, phantom, N_DST, Z, a1, tau, org)
    (out * v["dout"].to(dtype)).sum().backward()
    return dict(out=out.detach(), dZ=Z.grad, da1=a1.grad, dtau=tau.grad, dorigin=org.grad)


@functools.lru_cache(maxsize=None)
def autograd_refs(kind, order, H, D, regime, per_edge):
    _, arrays, v, _, _ = refs(kind, order, H, D, regime)
    o64, o32 = _oracle(arrays, v, H, D, torch.float64, per_edge), _oracle(arrays, v, H, D, torch.float32, per_edge)
    return o64, er.yardstick(o64, o32)


@pytest.mark.parametrize("variant,kind,H,D,regime,order", variant_cases())
def test_gat_aggregate_autograd(monkeypatch, variant, kind, H, D, regime, order):
    """ops.gat_aggregate, both tau modes, against oracle.fused.gat_aggregate_ref (fp64; its
    fp32 run is the yardstick): output and every gradient."""
    from hetersumgraph_amd.ops import HSG_TAU_PER_EDGE, HSG_TAU_TABLE, gat_aggregate
    skip_unless_dev(variant == "default")
    for k, x in VARIANTS[variant].items():
        monkeypatch.setenv(k, x)
    reld, arrays, v, _, _ = refs(kind, order, H, D, regime)
    tfl = torch.as_tensor(arrays[2]).long()
    for per_edge in (False, True):
        o64, yard = autograd_refs(kind, order, H, D, regime, per_edge)
        tau = v["tau"][tfl] if per_edge else v["tau"]
        dl = [dv(t).requires_grad_() for t in (v["Z"], v["a1"], tau, v["origin"])]
        out = gat_aggregate(*dl, reld, H, D, tau_mode=HSG_TAU_PER_EDGE if per_edge else HSG_TAU_TABLE)
        (out * dv(v["dout"])).sum().backward()
        torch.cuda.synchronize()
        entry = f"ops.gat_aggregate({'per-edge' if per_edge else 'table'})" + ("" if variant == "default" else f"[{variant}]")
        tag = rid(regime, order)
        compare(entry, tag, "out", out, o64["out"], yard["out"])
        for name, t in zip(("dZ", "da1", "dtau", "dorigin"), dl):
            compare(entry, tag, name, t.grad, o64[name], yard[name])


def _table_oracle(arrays, p, H, D, dtype):
    from oracle.fused import gat_aggregate_ref
    from test_gpu_ops import tau_table_ref
    e_src, e_dst, tf, phantom = arrays
    lv = {k: (t.to(dtype).clone().requires_grad_() if t is not None else None) for k, t in p.items() if k != "dout"}
    tau = tau_table_ref(lv["attn"], lv["T"], lv["wf"], lv["bf"], D)
    out = gat_aggregate_ref(e_src, e_dst, tf, phantom, N_DST, lv["Z"], lv["attn"][:, :D], tau, lv["origin"])
    (out * p["dout"].to(dtype)).sum().backward()
    r = {"out": out.detach(), "tau": tau.detach()}
    r.update({"d" + k: t.grad for k, t in lv.items() if t is not None})
    return r


@pytest.mark.parametrize("kind", ["short", "long", "long_wl"])
@pytest.mark.parametrize("H,D,bias", [(8, 8, False), (6, 50, True)])
@pytest.mark.parametrize("scale", ["unit", "trained"])
def test_gat_heads_table_autograd(kind, H, D, bias, scale):
    """The fused table path (hsg_attn_params_fwd / _bwd + the edge kernels): tau comes out of
    the layer's own parameters.  'trained': attn[:, 2D:] scaled per head so that the rows of
    tau_table_ref have rms 100 -- magnitudes of 50 to 150 and both signs, as unconstrained
    attn_fc / feat_fc weights may grow to -- which carries the table kernels and their
    backward through the same magnitudes."""
    from hetersumgraph_amd.ops import gat_heads_table
    from test_gpu_ops import tau_table_ref
    reld, *arrays = er.relation(kind)
    F = 50
    torch.manual_seed(er.SEED + 1)
    p = dict(Z=er.r64(N_SRC, H * D), attn=er.r64(H, 3 * D, scale=0.3), T=er.r64(10, F), wf=er.r64(H, D, F) / F ** 0.5,
             bf=er.r64(H, D, scale=0.2) if bias else None, origin=er.r64(N_DST, H * D), dout=er.r64(N_DST, H * D))
    if scale == "trained":
        t0 = tau_table_ref(p["attn"].double(), p["T"].double(), p["wf"].double(), p["bf"].double() if bias else None, D)
        p["attn"][:, 2 * D:] *= (100.0 / t0.pow(2).mean(0).sqrt()).float().unsqueeze(1)
    o64, o32 = _table_oracle(arrays, p, H, D, torch.float64), _table_oracle(arrays, p, H, D, torch.float32)
    yard = er.yardstick(o64, o32)
    if scale == "trained":
        assert 50 <= o64["tau"].abs().median() <= 150 and (o64["tau"] > 50).any() and (o64["tau"] < -50).any()
    dl = {k: (dv(t).requires_grad_() if t is not None else None) for k, t in p.items() if k != "dout"}
    out = gat_heads_table(dl["Z"], dl["attn"], dl["T"], dl["wf"], dl["bf"], dl["origin"], reld, H, D)
    (out * dv(p["dout"])).sum().backward()
    torch.cuda.synchronize()
    compare("ops.gat_heads_table", scale, "out", out, o64["out"], yard["out"])
    for k, t in dl.items():
        if t is not None:
            compare("ops.gat_heads_table", scale, "d" + k, t.grad, o64["d" + k], yard["d" + k])
