"""The row kernels of csrc/hsg_rows.hip against plain references: the dispatch table, the
seeded inputs of every numeric regime, the torch references and a numpy fp32 restatement
of the kernels' summation order.  Shared by tests/test_rows_cpu.py and
tests/test_gpu_rows.py.

Reference (module/GATLayer.py:40-42 of the original model):

    s   = keep * scale * y + x                    (keep: oracle.masks.ffn_keep, scale: ffn_scale)
    out = LayerNorm(s; gamma, beta, eps)          torch.native_layer_norm on the CPU

in fp64 and in fp32 on the same fp32 input values; the backward is autograd of
(out * dout).sum(): dx = grad x, dy = dx * keep * scale, dgamma, dbeta, db2 = dy.sum(0).

Tolerance convention (tests/test_gpu_lstm.py, tests/head_ref.py): a kernel may err by
FACTOR = 4 times ``yard``, the max |fp32 CPU - fp64| of the same quantity on the same
batch.  Rows whose elements are all equal (the ``constant`` regime, and every row at
d = 1) are the exception for out / mean / rstd: torch's fp32 LayerNorm is exact there
(yard = 0) while a tree of fp32 adds is not, so the bound is analytic (constant_bounds).
"""
import numpy as np
import torch

from oracle import masks

FACTOR = 4
EPS = 1e-5
OUT_ABS = 2e-5                 # tests/test_gpu_ffn.py's absolute bound on normal-regime outputs
MASK_SEED, MASK_OFFSET = 77, 9

SCALAR_WIDTHS = (1, 3, 7, 63, 65, 127, 130, 193, 255, 257, 323, 386, 449, 511)     # NPL 1..8
FORCED_WIDTHS = (64, 300)      # vector widths sent to the scalar kernels by a misaligned y (and dy)
VEC_WIDTHS = (4, 8, 64, 100, 252, 256)
PERSISTENT_WIDTHS = (260, 300, 508, 512)
BF16_WIDTHS = PERSISTENT_WIDTHS
ROWS = (1, 3, 4, 5, 7, 8, 9, 37)
# (d, aligned) of every parity case
WIDTH_CASES = tuple([(d, True) for d in SCALAR_WIDTHS] + [(d, False) for d in FORCED_WIDTHS] +
                    [(d, True) for d in VEC_WIDTHS + PERSISTENT_WIDTHS])

FWD_WRAPS = ((32773, 7), (6147, 260))                       # (n, d): one pass of the grid is 32,768 / 6,144 rows
BWD_WRAPS = tuple((n, d) for d in (7, 130, 260) for n in (2047, 2048, 2049, 4097, 6145))

# (regime, p, eps, outlier column: 0 first, -1 last)
REGIMES = tuple([(r, p, EPS, 0) for r in ("normal", "offset", "tiny", "huge", "outlier") for p in (0.0, 0.1)] +
                [("outlier", p, EPS, -1) for p in (0.0, 0.1)] +
                [("constant", 0.0, EPS, 0), ("normal", 0.5, EPS, 0), ("normal", 0.9, EPS, 0),
                 ("normal", 0.1, 1e-3, 0)])
# regimes where x_hat of some row is rounding noise scaled by up to eps^-1/2 = 316, or
# where one element carries the whole row: dgamma = sum dout * x_hat has an fp64 value
# far below its fp32 noise (1e-13 against 1e-3), so it is only required to be finite
DGAMMA_UNCHECKED = ("constant", "outlier")


# ------------------------------------------------------------------ dispatch
def family(entry, d, aligned):
    """The kernel family hsg_ln_fwd / hsg_ln_bwd (csrc/hsg_rows.hip, product build) launch
    for width d; ``aligned``: every pointer the host code tests is 16-byte aligned
    (forward: y, x, out, gamma, beta; backward: dout, y, x, gamma, dy, dx).

    forward  (entry "fwd"):
      d % 4 != 0 or a misaligned pointer -> "fwd_scalar<NPL>", NPL = ceil(d / 64):
          k_ln_fwd<NPL>, 4 rows per block, min(ceil(n/4), 8192) blocks, grid-stride loop
          (a second pass above 32,768 rows)
      d % 4 == 0, d <= 256, aligned     -> "fwd_vec<1,2>": k_ln_fwd4<1,2>, 8 rows per
          block (2 per wave), ceil(n/8) blocks, no loop
      d % 4 == 0, 257..512, aligned     -> "fwd_persistent<2,1>": k_ln_fwd4p<2,1>,
          min(1536, ceil(n/4)) blocks, one row per wave per pass (a second pass above
          6,144 rows), next row's loads in flight
    backward (entry "bwd"):
      d % 4 == 0, 257..512, aligned     -> "bwd_vec<2>": k_ln_bwd4p<2>
      everything else                   -> "bwd_scalar<NPL>": k_ln_bwd<NPL>, two rows of
          a wave's walk in flight
      both on min(ceil(n/4), 512) blocks = hsg_ln_bwd_blocks(n) (a second row per wave
      above 2,048 rows)."""
    assert 1 <= d <= 512
    npl = (d + 63) // 64
    quad = d % 4 == 0 and aligned
    if entry == "fwd":
        if not quad:
            return f"fwd_scalar<{npl}>"
        return "fwd_vec<1,2>" if d <= 256 else "fwd_persistent<2,1>"
    assert entry == "bwd"
    return "bwd_vec<2>" if quad and d > 256 else f"bwd_scalar<{npl}>"


def order_of(fam):
    """'quad' for the float4 kernels (lane owns columns 4*lane + 256*i + e), 'lane' for
    the scalar ones (lane owns columns lane + 64*i)."""
    return "lane" if "scalar" in fam else "quad"


def bwd_blocks(n):
    """hsg_ln_bwd_blocks(n) of the product build."""
    return min(max((n + 3) // 4, 1), 512)


# ------------------------------------------------------------------ inputs
def signed_gamma(d, g):
    """gamma ~ 1 + 0.1 randn with zeros (columns = 3 mod 5) and negated entries (columns
    = 5 mod 7): every width from 7 up has both."""
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).float()
    idx = torch.arange(d)
    gamma[idx % 5 == 3] = 0.0
    gamma[idx % 7 == 5] *= -1.0
    return gamma


def groups(d, n):
    """Independent launches per case.  yard is a maximum over the batch's elements, and with
    a handful of them (one row of three columns) it is a draw, not a yardstick: the CPU
    restatement of the kernels' order missed 4 x yard by up to 2.4x at d = 1, 3, 4, 7 with
    one launch per case, on dbeta (d samples) and on out at d = 3, and was inside it at
    every wider width.  So a case is G launches of n rows on independent data, with yard
    and the error both taken over all of them: at least 64 column sums and 32 rows."""
    return max(-(-64 // d), -(-32 // n))


def make_batch(d, n, regime="normal", p=0.0, eps=EPS, col=0, bf16=False, G=None):
    """fp32 inputs of one case: G launches of n rows each, stacked ([G * n, d]; launch g is
    rows g * n .. g * n + n - 1 and draws the same keep mask, which depends on the
    element index inside the launch).  s = keep * scale * y + x has the regime's shape:
      normal    y, x ~ N(0, 1/2): unit-variance rows
      offset    x = 1e3 + z, every row of z standardised to spread exactly 1, y ~ 0.1 N(0, 1):
                mean 1e3, spread 1.  (With x = 1e3 + N(0, 1/2) = y a three-column row now and
                then has a spread of 0.1 or less; at mean 1e3 its rstd carries rstd^3 * ulp(1e3)
                of error, one such row sets both yard and the error, and the restated order
                reached 6.2 x yard on rstd at d = 3, n = 8.  A floor on the spread removes the
                draw, not the regime.)
      tiny      y, x ~ 1e-4 N(0, 1): variance below eps
      huge      y, x ~ 1e15 N(0, 1) (the row's sum of squares stays inside fp32)
      outlier   normal with x[:, col] = 1e6 (col 0: first lane, col -1: last quad)
      constant  y = 0, x[r, :] = c_r with 0.25 <= |c_r| <= 2, row 0 all zero
    bf16: y and x are rounded to bf16 values first (the *16 entries read exactly these)."""
    G = groups(d, n) if G is None else G
    g = torch.Generator().manual_seed(1000003 * d + 101 * n + 7 * [r[0] for r in REGIMES].index(regime) +
                                      int(1000 * p) + (1 if col else 0))
    N = G * n
    y = torch.randn(N, d, generator=g)
    x = torch.randn(N, d, generator=g)
    if regime in ("normal", "outlier"):
        y, x = y * 0.5 ** 0.5, x * 0.5 ** 0.5
        if regime == "outlier":
            x[:, col] = 1e6
    elif regime == "offset":
        if d > 1:
            x = (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)
        y, x = y * 0.1, 1e3 + x
    elif regime == "tiny":
        y, x = y * 1e-4, x * 1e-4
    elif regime == "huge":
        y, x = y * 1e15, x * 1e15
    elif regime == "constant":
        c = (0.25 + 1.75 * torch.rand(N, generator=g)) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
        c[0] = 0.0
        y, x = torch.zeros(N, d), c[:, None].expand(N, d).clone()
    else:
        raise ValueError(regime)
    y, x = y.float().contiguous(), x.float().contiguous()
    if bf16:
        y, x = y.bfloat16().float(), x.bfloat16().float()
    keep = torch.from_numpy(masks.ffn_keep(MASK_SEED, MASK_OFFSET, n, d, p)) if p > 0 else torch.ones(n, d,
                                                                                                     dtype=torch.bool)
    return dict(G=G, n=n, d=d, regime=regime, p=p, eps=eps, y=y, x=x, gamma=signed_gamma(d, g),
                beta=(0.1 * torch.randn(d, generator=g)).float(), dout=torch.randn(N, d, generator=g).float(),
                keep=keep.repeat(G, 1), scale=masks.ffn_scale(p) if p > 0 else 1.0)


def constant_rows(b):
    """Every row of s has equal elements: the constant regime (s = c exactly), and d = 1."""
    return b["regime"] == "constant" or b["d"] == 1


# ------------------------------------------------------------------ torch references
def reference(b, dtype):
    """Forward and backward of one batch in ``dtype`` on the CPU: out, dx, dy [G * n, d],
    mean, rstd [G * n], dgamma, dbeta, db2 [G, d] (per launch: gamma and beta enter as one
    leaf row per launch, so autograd returns each launch's sums)."""
    G, n, d = b["G"], b["n"], b["d"]
    keep = b["keep"].to(dtype)
    x = b["x"].to(dtype).clone().requires_grad_()
    gamma = b["gamma"].to(dtype).expand(G, d).clone().requires_grad_()
    beta = b["beta"].to(dtype).expand(G, d).clone().requires_grad_()
    scale = torch.tensor(b["scale"], dtype=dtype)
    s = keep * (b["y"].to(dtype) * scale) + x
    if G == 1:
        out, mean, rstd = torch.native_layer_norm(s, (d,), gamma[0], beta[0], b["eps"])
    else:
        xh, mean, rstd = torch.native_layer_norm(s, (d,), None, None, b["eps"])
        out = xh * gamma.repeat_interleave(n, 0) + beta.repeat_interleave(n, 0)
    dx, dgamma, dbeta = torch.autograd.grad((out * b["dout"].to(dtype)).sum(), (x, gamma, beta))
    dy = dx * keep * scale
    r = dict(out=out.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), dx=dx, dy=dy,
             dgamma=dgamma, dbeta=dbeta, db2=dy.reshape(G, n, d).sum(1))
    return {k: v.double() for k, v in r.items()}


def references(b):
    """(fp64 reference, yard): yard[k] = max |fp32 CPU - fp64| of quantity k."""
    r64, r32 = reference(b, torch.float64), reference(b, torch.float32)
    return r64, {k: (r32[k] - r64[k]).abs().max().item() for k in r64}


def constant_bounds(b):
    """Analytic bounds for rows of equal elements c, s = c exactly (y = 0, p = 0).

    mu is reached from the d copies of c through at most K = 15 fp32 roundings: a lane
    adds its up to 8 columns one after another (8 adds; the quad kernels add 2 quads of 4
    in a tree of depth 4), the xor butterfly adds 6 levels, and the division by d is one
    more.  Every partial sum is a sum of copies of c, so its magnitude never exceeds the
    final one and each rounding moves the result by at most 2^-24 relative:
        |mean - c| <= K * 2^-24 * |c|.
    (The first lane add, 0 + c, is exact, so 14 roundings are live; the spare one absorbs
    the second-order terms and the roundings of the output's two products and add for the
    |gamma * c| >= 1/8 this module generates.)  s - mu is then exact or one more such
    step, rstd <= eps^-1/2, hence
        |out - beta| <= |gamma| * eps^-1/2 * K * 2^-24 * |c|,
    and var <= (K 2^-24 c)^2 << eps puts rstd within 1e-3 relative of eps^-1/2.
    At d = 1 (any regime) mu = s / 1 is the kernel's own fp32 s: mean keeps 4 x yard (the
    rounding of s is the reference's too), s - mu = 0 makes out = beta exactly, and var = 0
    puts rstd at eps^-1/2 as above; c = 0 selects exactly that here.
    Returns (mean bound [n], out bound [n, d], rstd target, rstd relative bound)."""
    K = 15
    c = b["x"].double()[:, 0].abs() * (0.0 if b["d"] == 1 else 1.0)
    bm = K * 2.0 ** -24 * c
    return bm, b["gamma"].double().abs()[None, :] * b["eps"] ** -0.5 * bm[:, None], b["eps"] ** -0.5, 1e-3


# ------------------------------------------------------------------ the kernels' order, fp32 numpy
F32 = np.float32


def _fma(a, b, c):
    """fmaf on fp32 arrays (the product is exact in fp64; the double rounding of the sum
    is below what this restatement is used for)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _lanes(a, d, order):
    """[n, d] -> [n, 64 lanes, 8 slots] in the order a lane meets its columns, and the
    validity of each slot.  lane: column lane + 64*i at slot i; quad: column
    4*lane + 256*i + e at slot 4*i + e."""
    n = a.shape[0]
    pad = np.zeros((n, 512), F32)
    pad[:, :d] = a
    ok = np.zeros(512, bool)
    ok[:d] = True
    if order == "lane":
        return pad.reshape(n, 8, 64).transpose(0, 2, 1), ok.reshape(8, 64).T[None]
    return (pad.reshape(n, 2, 64, 4).transpose(0, 2, 1, 3).reshape(n, 64, 8),
            ok.reshape(2, 64, 4).transpose(1, 0, 2).reshape(64, 8)[None])


def _unlanes(a, d, order):
    n = a.shape[0]
    if order == "lane":
        return a.transpose(0, 2, 1).reshape(n, 512)[:, :d]
    return a.reshape(n, 64, 2, 4).transpose(0, 2, 1, 3).reshape(n, 512)[:, :d]


def _wsum(v):
    """The 32..1 xor butterfly over [n, 64]; every lane ends with the same value."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return v[:, 0]


def _seq_sum(a):
    acc = np.zeros(a.shape[:2], F32)
    for i in range(a.shape[2]):
        acc = acc + a[:, :, i]
    return acc


def _seq_fma(a, b):
    acc = np.zeros(a.shape[:2], F32)
    for i in range(a.shape[2]):
        acc = _fma(a[:, :, i], b[:, :, i], acc)
    return acc


def _s_of(b):
    y, x, keep = b["y"].numpy(), b["x"].numpy(), b["keep"].numpy()
    v = np.where(keep, y * F32(b["scale"]), F32(0)) if b["p"] > 0 else y
    return (v + x).astype(F32)


def restated_fwd(b, order):
    """out, mean, rstd as k_ln_fwd (order 'lane') or k_ln_fwd4 / k_ln_fwd4p ('quad')
    compute them: per-lane partial sums, butterfly, two-pass variance with fmaf."""
    d = b["d"]
    with np.errstate(over="ignore", invalid="ignore"):
        s = _s_of(b)
        L, ok = _lanes(s, d, order)
        if order == "lane":
            acc = _seq_sum(L)
        else:
            acc = np.zeros(L.shape[:2], F32)
            for i in (0, 4):                                   # acc += (s0 + s1) + (s2 + s3) per quad
                acc = acc + ((L[:, :, i] + L[:, :, i + 1]) + (L[:, :, i + 2] + L[:, :, i + 3]))
        mu = _wsum(acc) / F32(d)
        t = np.where(ok, L - mu[:, None, None], F32(0))
        var = _wsum(_seq_fma(t, t)) / F32(d) + F32(b["eps"])
        rs = (1.0 / np.sqrt(var.astype(np.float64))).astype(F32)
        out = _fma((s - mu[:, None]) * rs[:, None], b["gamma"].numpy()[None, :], b["beta"].numpy()[None, :])
    return dict(out=out, mean=mu, rstd=rs)


def restated_bwd(b, order, mean, rstd):
    """dx, dy and each launch's block partials part[G][blocks][3][d] (dgamma, dbeta, db2) as k_ln_bwd /
    k_ln_bwd4p compute them from the forward's mean / rstd: wave w of the grid walks rows
    w, w + waves, ... accumulating its column partials in that order; a block adds its 4
    waves' partials in order."""
    n, d = b["n"], b["d"]                                      # rows per launch
    sc = F32(b["scale"])
    keep = b["keep"].numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        s = _s_of(b)
        mu, rs = mean.astype(F32)[:, None], rstd.astype(F32)[:, None]
        xh = (s - mu) * rs
        go = b["dout"].numpy()
        g = go * b["gamma"].numpy()[None, :]
        Lg, ok = _lanes(g, d, order)
        Lx, _ = _lanes(xh, d, order)
        mg = (_wsum(_seq_sum(Lg)) / F32(d))[:, None]
        mgx = (_wsum(_seq_fma(Lg, Lx)) / F32(d))[:, None]
        dx = rs * _fma(-xh, np.broadcast_to(mgx, xh.shape), g - mg)
        dy = np.where(keep, dx * sc, F32(0)).astype(F32)
        blocks = bwd_blocks(n)
        waves = 4 * blocks
        acc = np.zeros((b["G"], 3, waves, d), F32)
        for q in range(b["G"]):
            for r0 in range(0, n, waves):
                m = min(waves, n - r0)
                lo = q * n + r0
                acc[q, 0, :m] = _fma(go[lo:lo + m], xh[lo:lo + m], acc[q, 0, :m])
                acc[q, 1, :m] = acc[q, 1, :m] + go[lo:lo + m]
                acc[q, 2, :m] = acc[q, 2, :m] + dy[lo:lo + m]
        w = acc.reshape(b["G"], 3, blocks, 4, d)
        part = (((w[:, :, :, 0] + w[:, :, :, 1]) + w[:, :, :, 2]) + w[:, :, :, 3]).transpose(0, 2, 1, 3)
    return dict(dx=dx.astype(F32), dy=dy, part=np.ascontiguousarray(part))


def restated_colsums(P):
    """k_ffn_colsums on a slab P [rows, cols]: row group g = r mod 8 adds its rows in four
    interleaved accumulators (steps of 32 rows) with the tail in the first, pairs them,
    and the 8 group sums are added in order."""
    rows, cols = P.shape
    red = np.zeros((8, cols), F32)
    for g in range(8):
        s = np.zeros((4, cols), F32)
        r = g
        while r + 24 < rows:
            for q in range(4):
                s[q] = s[q] + P[r + 8 * q]
            r += 32
        while r < rows:
            s[0] = s[0] + P[r]
            r += 8
        red[g] = (s[0] + s[1]) + (s[2] + s[3])
    a = np.zeros(cols, F32)
    for g in range(8):
        a = a + red[g]
    return a


def seq_colsum32(P):
    """Sequential fp32 column sum (the yardstick of the hsg_ffn_colsums test)."""
    a = np.zeros(P.shape[1], F32)
    for r in range(P.shape[0]):
        a = a + P[r]
    return a
