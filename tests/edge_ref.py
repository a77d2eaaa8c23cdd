"""The edge kernels' operation restated once, for every test that calls them directly
(tests/test_gpu_guard_bands.py, tests/test_gpu_logit_range.py, tests/test_logit_regimes.py).

* the three guard-band relations (97 sources, 61 destinations) and their inputs;
* the logit regimes: ways of drawing ``tau`` (and ``a1`` for one of them) that move the
  post-LeakyReLU logits away from zero, where softmax's shift-invariance no longer hides
  the max subtraction, the initial running maximum and the rescale steps;
* ``restate``: forward and backward of one edge-softmax application from the formulas of
  include/hsg.h, in any dtype -- fp64 is the reference, the same code in fp32 on the CPU is
  the yardstick an fp32 kernel is measured with (``yardstick``, ``allowed``).

Regime ``unit`` draws exactly what the guard-band cases have always drawn.
"""
import functools

import numpy as np
import torch

from helpers import random_relation
from oracle.fused import phantom_term

DEV = "cuda"
N_SRC, N_DST = 97, 61
LONG_DST = 30                                # the destination with the long segment
SEED = 20240                                 # test_gpu_guard_bands.run_case seeds the same

# tolerance of the edge forward: test_gpu_ops.py::test_gat_aggregate_matches_op_restatement (2e-5 absolute)
GAT_TOL = (2e-5, 0.0)

REGIMES = ("unit", "offset+", "offset-", "spread", "ties")
SPREAD_ROWS = (-2e4, -1e4, -3e3, -100.0, 0.0, 20.0, 45.0, 88.0, 89.0, 120.0, 150.0)


def r64(*shape, scale=1.0):
    """fp32-representable random values as a CPU fp32 tensor (the seeded default generator)."""
    return torch.randn(*shape) * scale


def ops_tol(ref):
    return (2e-5 * max(1.0, ref.abs().max().item()), 0.0)


def apply_regime(regime, g, a1):
    """(tau, a1) of a regime from the standard-normal table g [11, H] and the unit regime's
    a1, both fp32; formed in fp64 and rounded to fp32 once."""
    if regime == "unit":
        return g, a1
    gd = g.double()
    if regime == "offset+":                  # every logit about 100, O(1) differences
        t = 100.0 + gd
    elif regime == "offset-":                # post-leaky about -120 +- 1
        t = -1.2e4 + 100.0 * gd
    elif regime == "spread":                 # saturated softmax, maxima 30 .. 150 apart
        t = torch.tensor(SPREAD_ROWS, dtype=torch.float64).unsqueeze(1) + gd
    elif regime == "ties":                   # all logits equal and large
        return torch.full_like(g, 100.0), torch.zeros_like(a1)
    else:
        raise ValueError(regime)
    return t.float(), a1


# ------------------------------------------------------------------------------------
# relations of the edge kernels: 97 sources, 61 destinations (no multiple of 4 or of the
# nodes per block); the LAST destination has no typed edge (phantoms only), destination 7
# only phantoms, destination 13 no in-edge at all, destination 30 a long segment
@functools.lru_cache(maxsize=None)
def relation_host(kind, order=None):
    """'short': mean segment < 16 (one wave per destination); 'long': mean >= 16 (4 waves
    per destination); 'long_wl': 'long' built with work lists.  order 'asc' / 'desc': the
    long destination's tf rows sorted, so that under regime 'spread' its maximum arrives in
    the last / the first batch or piece."""
    def make(tf=None):
        rng = np.random.default_rng(61 if kind == "short" else 97)
        if kind == "short":
            deg = rng.integers(0, 6, size=N_DST)
            deg[LONG_DST] = 90
        else:
            deg = rng.integers(10, 41, size=N_DST)
            deg[LONG_DST] = 200
        phantom = rng.integers(0, 4, size=N_DST)
        deg[[7, 13, N_DST - 1]] = 0
        phantom[7], phantom[13], phantom[N_DST - 1] = 3, 0, 2
        return random_relation(rng, N_SRC, N_DST, 0, deg=deg, phantom=phantom, tf=tf)
    out = make()
    if order is not None:
        rel, e_src, e_dst, tf, phantom = out
        seg = np.nonzero(e_dst == LONG_DST)[0]
        tf = tf.copy()
        tf[seg] = np.sort(tf[seg])[::1 if order == "asc" else -1]
        out = make(tf)
        assert np.array_equal(out[1], e_src) and np.array_equal(out[2], e_dst)
    return out


@functools.lru_cache(maxsize=None)
def relation(kind, order=None):
    """relation_host on the device; 'long_wl' with CSR / CSC work lists of a small piece length."""
    from hetersumgraph_amd import _lib
    rel, e_src, e_dst, tf, phantom = relation_host(kind, order)
    with _lib.path_options(HSG_PIECE_MIN="8" if kind == "long_wl" else "0"):
        reld = rel.to(DEV)
    torch.cuda.synchronize()
    assert ("dwork" in reld.dev) == (kind == "long_wl") and ("swork" in reld.dev) == (kind == "long_wl")
    return reld, e_src, e_dst, tf, phantom


def draw(H, D, regime="unit", dout=False):
    """The inputs of one application, in the order the guard-band cases draw them."""
    HD = H * D
    v = dict(Z=r64(N_SRC, HD), a1=r64(H, D, scale=0.3), tau=r64(11, H), origin=r64(N_DST, HD))
    if dout:
        v["dout"] = r64(N_DST, HD)
    v["tau"], v["a1"] = apply_regime(regime, v["tau"], v["a1"])
    return v


def restate(arrays, v, H, D, dtype=torch.float64, g_bf16=False, om=1, given=None):
    """Forward and backward of one application from hsg.h's formulas, in ``dtype``.
    arrays = (e_src, e_dst, tf, phantom); v: fp32 CPU tensors Z, a1, tau [11, H], origin and
    (for the backward) dout.  Returns (r, handed): r the results in ``dtype``; handed the
    fp32 / bf16 tensors derived from the fp64 run that a kernel is handed as inputs.

    given: the intermediate results a backward entry point is handed instead of computing
    them -- any of m, l, h, G, rho, dpre (fp32) -- so that the run restates that entry point
    from ITS inputs: the backward then continues from these values, as the kernel does.

    m_v = max(max_e s_e, 0 if phantom_v > 0), l_v = sum_e exp(s_e - m_v) + phantom_v exp(-m_v);
    (m_saved, l_saved): a destination without a typed in-edge -- phantoms or not -- stores
    (0, 1), as hsg.h says (no edge reads them: alpha = exp(s - m) / l is per typed edge)."""
    e_src, e_dst, tf, phantom = arrays
    HD = H * D
    es, ed, tfl = torch.as_tensor(e_src).long(), torch.as_tensor(e_dst).long(), torch.as_tensor(tf).long()
    Z, a1, tau = v["Z"].to(dtype), v["a1"].to(dtype), v["tau"].to(dtype)
    handed = {"sigma": (Z.view(N_SRC, H, D) * a1).sum(-1).float()}
    sigma = handed["sigma"].to(dtype)
    pre = sigma[es] + tau[tfl]
    s_ = torch.where(pre > 0, pre, 0.01 * pre)
    ph = torch.as_tensor(phantom).to(dtype).unsqueeze(1)
    m = torch.full((N_DST, H), -torch.inf, dtype=dtype).scatter_reduce(0, ed.unsqueeze(1).expand(-1, H), s_, "amax")
    m = torch.where(ph > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    pe = torch.exp(s_ - m[ed])
    l = torch.zeros(N_DST, H, dtype=dtype).index_add(0, ed, pe) + phantom_term(ph, m)
    typed = torch.zeros(N_DST, dtype=torch.bool).index_fill(0, ed, True).unsqueeze(1)
    r = dict(sigma=sigma, m_saved=torch.where(typed, m, torch.zeros_like(m)),
             l_saved=torch.where(typed, l, torch.ones_like(l)))
    l = torch.where(l == 0, torch.ones_like(l), l)          # no in-edge at all: the forward stores (0, 1)
    given = given or {}
    take = lambda k, own: given[k].to(dtype).reshape(own.shape) if k in given else own
    if "m" in given or "l" in given:
        m, l = take("m", m), take("l", l)
        pe = torch.exp(s_ - m[ed])
    alpha = pe / l[ed]                                      # [E, H]
    Zh = Z.view(N_SRC, H, D)
    h = torch.zeros(N_DST, H, D, dtype=dtype).index_add(0, ed, alpha.unsqueeze(-1) * Zh[es])
    hf = h.view(N_DST, HD)
    x = torch.nn.functional.elu(hf) + v["origin"].to(dtype)
    r.update(h=hf, m=m, l=l, x=x, alpha=alpha)
    if "dout" not in v:
        return r, handed
    hf = take("h", hf)
    h = hf.view(N_DST, H, D)
    G = v["dout"].to(dtype) * (torch.where(hf > 0, torch.ones_like(hf), torch.exp(hf)) if om else 1.0)   # om 0: out = h
    G = take("G", G)
    if g_bf16:
        handed["G16"] = G.float().bfloat16()
        Gu = handed["G16"].to(dtype)
    else:
        Gu = G.float().to(dtype)                            # the G rows the kernels are handed
    Gh = Gu.view(N_DST, H, D)
    rho = take("rho", (G.view(N_DST, H, D) * h).sum(-1))    # G_v . h_v per head (from the fp32 G)
    lk = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.01))
    dpre = take("dpre", alpha * ((Gh[ed] * Zh[es]).sum(-1) - rho[ed]) * lk)
    dsigma = torch.zeros(N_SRC, H, dtype=dtype).index_add(0, es, dpre)
    dZ0 = torch.zeros(N_SRC, H, D, dtype=dtype).index_add(0, es, alpha.unsqueeze(-1) * Gh[ed])
    dZ = (dZ0 + dsigma.unsqueeze(-1) * a1).view(N_SRC, HD)
    dtau = torch.zeros(11, H, dtype=dtype).index_add(0, tfl, dpre)
    da1 = (dsigma.unsqueeze(-1) * Zh).sum(0).view(HD)
    r.update(G=G, dpre=dpre, dsigma=dsigma, dZ0=dZ0.view(N_SRC, HD), dZ=dZ, dtau=dtau.view(-1), da1=da1, rho=rho)
    # rho[v][g][s]: the 64-column-group partials of G_v . h_v, head 64 g / D + s
    ng = (HD + 63) // 64
    rg = torch.zeros(N_DST, ng, 3, dtype=dtype)
    prod = G * hf
    for g in range(ng if D >= 32 else 0):                   # (wide heads only: at most 3 heads per group)
        for c in range(64 * g, min(64 * g + 64, HD)):
            rg[:, g, c // D - (64 * g) // D] += prod[:, c]
    r["rho_groups"] = rg
    return r, handed


def ties_closed_form(arrays, Z, H, D):
    """Regime 'ties' (every logit 100): alpha = 1 / (deg + phantom e^-100), so h is the
    segment sum of Z over deg + phantom e^-100 -- the segment mean.  fp64 [N_DST, H D]."""
    e_src, e_dst, _, phantom = arrays
    es, ed = torch.as_tensor(e_src).long(), torch.as_tensor(e_dst).long()
    deg = torch.zeros(N_DST, dtype=torch.float64).index_add(0, ed, torch.ones(len(ed), dtype=torch.float64))
    den = deg + torch.as_tensor(phantom).double() * np.exp(-100.0)
    tot = torch.zeros(N_DST, H * D, dtype=torch.float64).index_add(0, ed, Z.double()[es])
    return tot / torch.where(den == 0, torch.ones_like(den), den).unsqueeze(1)


# ------------------------------------------------------------------------------------
# what the guard-band cases use (regime 'unit': their inputs, bounds and assertions as before)
def ml_refs(arrays, sigma, tau, H):
    """The saved (m, l) of hsg.h in fp64 with the guard-band tolerances: the outputs' for m,
    relative to the largest entry for the sums l."""
    e_src, e_dst, tf, phantom = arrays
    es, ed, tfl = (torch.as_tensor(a).long() for a in (e_src, e_dst, tf))
    pre = sigma.double()[es] + tau.double()[tfl]
    s_ = torch.where(pre > 0, pre, 0.01 * pre)
    ph = torch.as_tensor(phantom).double().unsqueeze(1)
    m = torch.full((N_DST, H), -torch.inf, dtype=torch.float64).scatter_reduce(
        0, ed.unsqueeze(1).expand(-1, H), s_, "amax")
    m = torch.where(ph > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    l = torch.zeros(N_DST, H, dtype=torch.float64).index_add(0, ed, torch.exp(s_ - m[ed])) + phantom_term(ph, m)
    typed = torch.zeros(N_DST, dtype=torch.bool).index_fill(0, ed, True).unsqueeze(1)
    m, l = torch.where(typed, m, torch.zeros_like(m)), torch.where(typed, l, torch.ones_like(l))
    return {"m": (m, *GAT_TOL), "l": (l, GAT_TOL[0] * max(1.0, l.abs().max().item()), 0.0)}


def gat_fwd_inputs(kind, H, D, regime="unit"):
    from oracle.fused import gat_aggregate_ref
    reld, e_src, e_dst, tf, phantom = relation(kind)
    v = draw(H, D, regime)
    Z, a1, tau, origin = v["Z"], v["a1"], v["tau"], v["origin"]
    sigma = (Z.double().view(N_SRC, H, D) * a1.double()).sum(-1).float()
    h_ref = gat_aggregate_ref(e_src, e_dst, tf, phantom, N_DST, Z.double(), a1.double(), tau.double())
    x_ref = torch.nn.functional.elu(h_ref) + origin.double()
    return reld, Z, sigma, tau, origin, h_ref, x_ref, ml_refs((e_src, e_dst, tf, phantom), sigma, tau, H)


def gat_bwd_ref(kind, H, D, g_bf16=False, om=1, regime="unit"):
    """(relation, inputs v, fp64 results r, E): the header's formulas on the forward's fp64
    (h, m, l)."""
    reld, e_src, e_dst, tf, phantom = relation(kind)
    v = draw(H, D, regime, dout=True)
    r, handed = restate((e_src, e_dst, tf, phantom), v, H, D, torch.float64, g_bf16, om)
    v.update(handed)
    return reld, v, r, len(e_src)


# ------------------------------------------------------------------------------------
# the yardstick
def yardstick(r64_, r32):
    """name -> max-abs error of the fp32 run of the restatement against its fp64 run."""
    return {k: (r32[k].double() - r64_[k]).abs().max().item() if r64_[k].numel() else 0.0 for k in r64_}


def existing_bound(name, ref):
    """Today's bound of a compared tensor: 2e-5 absolute for h / out / m, 2e-5 max(1, |ref|_max)
    for l and the gradients."""
    if name in ("h", "x", "out", "x16", "m", "m_saved", "sigma"):
        return GAT_TOL[0]
    return 2e-5 * max(1.0, ref.abs().max().item() if ref.numel() else 0.0)


def allowed(name, ref, yard):
    """max(existing bound, 4 x yard): the factor tests/test_gpu_lstm.py grants a kernel whose
    summation order differs from torch's."""
    return max(existing_bound(name, ref), 4.0 * yard)
