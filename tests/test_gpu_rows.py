"""The row kernels of csrc/hsg_rows.hip through the C ABI against fp64, at every width class,
dispatch family and numeric regime of tests/rows_ref.py (the product library: the family
is chosen by d and pointer alignment alone, rows_ref.family).

Tolerances: 4 x yard (yard = max |fp32 CPU - fp64| of the same quantity on the same
batch, never taken from the kernels), the analytic bound on rows of equal elements
(rows_ref.constant_bounds), 2e-5 absolute on normal-regime outputs (tests/test_gpu_ffn.py)
and bitwise equality.  tests/test_rows_cpu.py shows on the CPU that the kernels' summation
order meets these bounds on exactly these inputs.

Mutations these cases catch (none is committed):
  * the forward's quad clamp min(4*lane + 256*i, d - 4) four columns low: the live quad at
    d - 4 loads d - 8 -- out, mean and rstd of every persistent case but d = 512, first at
    d = 260, n = 1.  Four columns high only reads past the last row, and the backward's
    clamp feeds only lanes whose loads are unused: no value moves, so no value test sees
    those (tests/test_gpu_guard_bands.py watches the written extent);
  * reading row n - 1 into a stored row (k_ln_fwd4's min(row0 + q, n - 1) applied to a
    live row): every fwd_vec<1,2> case with n >= 2, first at d = 4, n = 3;
  * dropping the second in-flight row's rr < n test in k_ln_bwd: rows n .. of dx / dy get
    written -- the NaN guard rows behind dx and dy in every backward case with n <= 2,048
    (first at d = 1, n = 1), and dbeta doubles where dout is read for it too.
"""
import numpy as np
import pytest
import torch

import rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from hetersumgraph_amd._lib import load
    return load()


def _dev(t, misalign=False):
    """Device copy; misalign: a view that starts one float past a 16-byte boundary."""
    t = t.contiguous()
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _nan(shape, misalign=False, dtype=torch.float32):
    return _dev(torch.full(shape, float("nan"), dtype=dtype), misalign)


def _seed(b):
    return torch.tensor([R.MASK_SEED], dtype=torch.int64, device=DEV) if b["p"] > 0 else None


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def run_fwd(b, misalign=False):
    """hsg_ln_fwd on each launch of the batch; device tensors (the backward reads them)."""
    lib, G, n, d = _lib(), b["G"], b["n"], b["d"]
    t = dict(y=_dev(b["y"], misalign), x=_dev(b["x"]), gamma=_dev(b["gamma"]), beta=_dev(b["beta"]),
             out=_nan((G * n, d)), mean=_nan((G * n,)), rstd=_nan((G * n,)), seed=_seed(b))
    for q in range(G):
        o, r = 4 * q * n * d, 4 * q * n
        rc = lib.hsg_ln_fwd(n, d, _p(t["y"], o), _p(t["x"], o), _p(t["gamma"]), _p(t["beta"]), b["eps"], b["p"],
                            _p(t["seed"]), R.MASK_OFFSET, _p(t["out"], o), _p(t["mean"], r), _p(t["rstd"], r), None)
        assert rc == 0, (rc, n, d)
    torch.cuda.synchronize()
    return t


def run_bwd(b, f, misalign=False):
    """hsg_ln_bwd on each launch with the mean / rstd its forward wrote (the product's chain),
    then hsg_ffn_colsums on its partials.  dx and dy carry one grid pass of NaN guard
    rows behind every launch: the rows a second in-flight row would hit."""
    lib, G, n, d = _lib(), b["G"], b["n"], b["d"]
    nb = lib.hsg_ln_bwd_blocks(n)
    assert nb == R.bwd_blocks(n)
    pitch = n + 4 * nb
    dout = _dev(b["dout"])
    dy, dx = _nan((G, pitch, d), misalign), _nan((G, pitch, d))
    part, sums = _nan((G, nb, 3, d)), _nan((G, 3, d))
    for q in range(G):
        o, r, og = 4 * q * n * d, 4 * q * n, 4 * q * pitch * d
        rc = lib.hsg_ln_bwd(n, d, _p(dout, o), _p(f["y"], o), _p(f["x"], o), _p(f["gamma"]), _p(f["mean"], r),
                            _p(f["rstd"], r), b["p"], _p(f["seed"]), R.MASK_OFFSET, _p(dy, og), _p(dx, og),
                            _p(part, 4 * q * nb * 3 * d), None)
        assert rc == 0, (rc, n, d)
        rc = lib.hsg_ffn_colsums(0, 0, None, None, nb, d, _p(part, 4 * q * nb * 3 * d), _p(sums, 4 * q * 3 * d),
                                 _p(sums, 4 * (q * 3 + 1) * d), _p(sums, 4 * (q * 3 + 2) * d), 0, None)
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(dx[:, n:]).all() and torch.isnan(dy[:, n:]).all(), ("rows past n written", n, d)
    return dict(dx=dx[:, :n].reshape(G * n, d), dy=dy[:, :n].reshape(G * n, d), part=part, sums=sums)


def _err(t, ref):
    return (t.detach().cpu().double() - ref).abs().max().item()


class Worst:
    """The worst err / yard of each quantity over the cases of one printed line."""

    def __init__(self):
        self.w = {}

    def add(self, k, err, yard):
        if yard > 0 and err / yard >= self.w.get(k, (-1.0,))[0]:
            self.w[k] = (err / yard, err, yard)

    def line(self, head):
        print(head + " " + "  ".join(f"{k} err {e:.3e} yard {y:.3e} ratio {r:.2f}" for k, (r, e, y) in self.w.items()))


def check_fwd(b, f, r64, yard, worst, what):
    if R.constant_rows(b):
        bm, bo, rs0, rs_rel = R.constant_bounds(b)
        if b["d"] == 1:
            e = _err(f["mean"], r64["mean"])
            worst.add("mean", e, yard["mean"])
            assert e <= R.FACTOR * yard["mean"], (what, "mean", e, yard["mean"])
        else:
            assert ((f["mean"].cpu().double() - r64["mean"]).abs() <= bm).all(), (what, "mean")
        assert ((f["out"].cpu().double() - r64["out"]).abs() <= bo).all(), (what, "out")
        assert ((f["rstd"].cpu().double() / rs0 - 1).abs() <= rs_rel).all(), (what, "rstd")
        return
    for k in ("out", "mean", "rstd"):
        e = _err(f[k], r64[k])
        worst.add(k, e, yard[k])
        assert yard[k] > 0 and e <= R.FACTOR * yard[k], (what, k, e, yard[k])
    if b["regime"] == "normal":
        assert _err(f["out"], r64["out"]) <= R.OUT_ABS, what


def check_bwd(b, g, r64, yard, worst, what):
    host = g["part"].cpu().double().sum(1)                     # [G, 3, d]: the partials summed in fp64
    sums = g["sums"]                                           # hsg_ffn_colsums of the same partials
    got = dict(dx=g["dx"], dy=g["dy"])
    for i, k in enumerate(("dgamma", "dbeta", "db2")):
        got[k], got[k + "(colsums)"] = host[:, i], sums[:, i]
    for k, v in got.items():
        base = k.split("(")[0]
        if base == "dgamma" and b["regime"] in R.DGAMMA_UNCHECKED:
            assert torch.isfinite(v).all(), (what, k)
            continue
        e = _err(v, r64[base])
        worst.add(k, e, yard[base])
        assert e <= R.FACTOR * yard[base], (what, k, e, yard[base])


# ------------------------------------------------------------------ parity with fp64
@pytest.mark.parametrize("d,aligned", R.WIDTH_CASES)
def test_rows_match_fp64(d, aligned):
    """Forward (out, mean, rstd) and backward (dx, dy, the block partials summed on the host
    and by hsg_ffn_colsums) of every regime and row count at one width.  aligned = False:
    y (and dy) start one float past a 16-byte boundary, which the host code of hsg_ln_fwd /
    hsg_ln_bwd answers with the scalar kernels (scalar loads and stores only)."""
    fam = R.family("fwd", d, aligned), R.family("bwd", d, aligned)
    for regime, p, eps, col in R.REGIMES:
        wf, wb = Worst(), Worst()
        for n in R.ROWS:
            b = R.make_batch(d, n, regime, p, eps, col)
            r64, yard = R.references(b)
            what = (d, n, regime, p, eps, col)
            f = run_fwd(b, misalign=not aligned)
            check_fwd(b, f, r64, yard, wf, what)
            check_bwd(b, run_bwd(b, f, misalign=not aligned), r64, yard, wb, what)
        tag = f"d {d} {regime} p {p} eps {eps} col {col}"
        wf.line(f"{fam[0]} {tag}:")
        wb.line(f"{fam[1]} {tag}:")


@pytest.mark.parametrize("n,d", R.FWD_WRAPS)
def test_forward_grid_wrap(n, d):
    """One pass of the forward's grid does not cover n: rows of the second pass."""
    b = R.make_batch(d, n, "normal", 0.1, G=1)
    r64, yard = R.references(b)
    w = Worst()
    check_fwd(b, run_fwd(b), r64, yard, w, (n, d))
    w.line(f"{R.family('fwd', d, True)} wrap n {n} d {d}:")


@pytest.mark.parametrize("n,d", R.BWD_WRAPS)
def test_backward_grid_wrap(n, d):
    """Around the backward's 512-block cap: the second in-flight row r0 + stride exists for
    no wave (n <= 2048), for one (2049), for every wave (4097: and a third row for one),
    and a fourth row whose partner does not exist (6145)."""
    b = R.make_batch(d, n, "normal", 0.1, G=1)
    r64, yard = R.references(b)
    w = Worst()
    check_bwd(b, run_bwd(b, run_fwd(b)), r64, yard, w, (n, d))
    w.line(f"{R.family('bwd', d, True)} wrap n {n} d {d}:")


def test_backward_of_no_rows_zeroes_its_partials():
    lib, d = _lib(), 300
    nb = lib.hsg_ln_bwd_blocks(0)
    assert nb == 1
    part = _nan((nb, 3, d))
    assert lib.hsg_ln_bwd(0, d, None, None, None, None, None, None, 0.0, None, 0, None, None, _p(part), None) == 0
    torch.cuda.synchronize()
    assert not part.any()


# ------------------------------------------------------------------ hsg_ffn_colsums
def _colsums(lib, hp, lp, pre, acc):
    rows_h, d_hid = hp.shape if hp is not None else (0, 0)
    rows_ln, d = (lp.shape[0], lp.shape[2]) if lp is not None else (0, 0)
    outs = [_dev(t) if t is not None else None for t in pre]
    # an empty slab still needs a pointer: the entry refuses NULL for a half that has columns
    slab = lambda t: None if t is None else (_dev(t) if t.numel() else torch.zeros(1, device=DEV))
    hpd, lpd = slab(hp), slab(lp)
    rc = lib.hsg_ffn_colsums(rows_h, d_hid, _p(hpd), _p(outs[0]), rows_ln, d, _p(lpd), _p(outs[1]), _p(outs[2]),
                             _p(outs[3]), acc, None)
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu() if o is not None else None for o in outs]


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 31, 32, 33, 57, 512])
def test_colsums_match_fp64(rows):
    """Column sums of random slabs against fp64; yard from a sequential fp32 column sum on
    the CPU.  Every column of every (d_hid, d) here is the same quantity -- a sum of
    ``rows`` N(0, 1) draws, plus an N(0, 1) prefill under accumulate -- so err and yard are
    taken over all of them per accumulate mode (d = 1 alone would be three samples)."""
    lib = _lib()
    g = torch.Generator().manual_seed(rows)
    for acc in (0, 1):
        err = yard = 0.0
        for d_hid in (1, 33, 100, 512):
            for d in (1, 7, 64, 300):
                hp, lp = torch.randn(rows, d_hid, generator=g), torch.randn(rows, 3, d, generator=g)
                pre = [torch.randn(k, generator=g) for k in (d_hid, d, d, d)]
                got = _colsums(lib, hp, lp, pre, acc)
                for o, pr, P in zip(got, pre, (hp, lp[:, 0], lp[:, 1], lp[:, 2])):
                    ref = P.double().sum(0) + (pr.double() if acc else 0)
                    s32 = R.seq_colsum32(P.numpy())
                    s32 = (pr.numpy() + s32) if acc else s32
                    err = max(err, (o.double() - ref).abs().max().item())
                    yard = max(yard, np.abs(s32.astype(np.float64) - ref.numpy()).max())
        print(f"hsg_ffn_colsums rows {rows} accumulate {acc}: err {err:.3e} yard {yard:.3e} "
              f"ratio {err / yard if yard else 0:.2f}")
        assert err <= R.FACTOR * yard, (rows, acc, err, yard)


def _col_ok(o, P):
    ref = P.double().sum(0)
    yard = np.abs(R.seq_colsum32(P.numpy()).astype(np.float64) - ref.numpy()).max()
    return (o.double() - ref).abs().max().item() <= R.FACTOR * yard


def test_colsums_absent_halves_and_no_rows():
    lib = _lib()
    g = torch.Generator().manual_seed(3)
    hp, lp = torch.randn(9, 33, generator=g), torch.randn(9, 3, 7, generator=g)
    pre = [torch.randn(k, generator=g) for k in (33, 7, 7, 7)]
    # d = 0: only db1; the LayerNorm outputs are not touched (and may be absent)
    got = _colsums(lib, hp, None, pre, 0)
    assert _col_ok(got[0], hp)
    assert all(torch.equal(a, b) for a, b in zip(got[1:], pre[1:]))
    assert _colsums(lib, hp, None, [pre[0], None, None, None], 0)[0].equal(got[0])
    # d_hid = 0: only dgamma, dbeta, db2
    got = _colsums(lib, None, lp, pre, 0)
    assert torch.equal(got[0], pre[0])
    for i in range(3):
        assert _col_ok(got[1 + i], lp[:, i])
    assert all(a.equal(b) for a, b in zip(_colsums(lib, None, lp, [None] + pre[1:], 0)[1:], got[1:]))
    assert lib.hsg_ffn_colsums(0, 0, None, None, 0, 0, None, None, None, None, 0, None) == 0
    # no rows: zeros, or the outputs unchanged under accumulate
    for acc in (0, 1):
        got = _colsums(lib, hp[:0], lp[:0], pre, acc)
        for o, pr in zip(got, pre):
            assert torch.equal(o, pr if acc else torch.zeros_like(pr))


# ------------------------------------------------------------------ the bf16 entries
def _bf16_rows(t, ld):
    """bf16 rows of pitch ld holding t (bf16-valued fp32); the pad is NaN: no entry reads it."""
    buf = _nan((t.shape[0], ld), dtype=torch.bfloat16)
    buf[:, :t.shape[1]] = t.to(DEV).bfloat16()
    return buf


@pytest.mark.parametrize("d", R.BF16_WIDTHS)
def test_bf16_entries_bitwise(d):
    """hsg_ln_fwd_y16 / _x16 and hsg_ln_bwd_dy16 / _x16 are the fp32 entries' templates with
    a conversion at the load (and at dy's store): on bf16-valued inputs every fp32 output
    is bitwise that of hsg_ln_fwd / hsg_ln_bwd, dy is the RNE bf16 of the fp32 dy, the pad
    columns d .. ceil8(d) - 1 are zero and the columns behind them keep their NaN.  The
    fp32 call itself is held to fp64 on the same bf16-valued inputs."""
    from hetersumgraph_amd._lib import load
    lib = load()
    ld0 = (d + 7) // 8 * 8
    for n in (1, 5, 37, 6147):
        for p in (0.0, 0.1):
            b = R.make_batch(d, n, "normal", p, bf16=True, G=1)
            f = run_fwd(b)
            if n >= 37:                                        # enough rows for a yardstick
                r64, yard = R.references(b)
                w = Worst()
                check_fwd(b, f, r64, yard, w, (d, n, p, "bf16 values"))
                w.line(f"hsg_ln_fwd on bf16 values d {d} n {n} p {p}:")
            seed, g = f["seed"], run_bwd(b, f)
            dout = _dev(b["dout"])
            yb = _dev(b["y"]).bfloat16()
            nb = lib.hsg_ln_bwd_blocks(n)
            for ld in (ld0, ld0 + 8):
                xb = _bf16_rows(b["x"], ld)
                for x16 in (False, True):
                    out, mean, rstd = _nan((n, d)), _nan((n,)), _nan((n,))
                    if x16:
                        rc = lib.hsg_ln_fwd_x16(n, d, _p(yb), _p(xb), ld, _p(f["gamma"]), _p(f["beta"]), b["eps"], p,
                                                _p(seed), R.MASK_OFFSET, _p(out), _p(mean), _p(rstd), None)
                    else:
                        rc = lib.hsg_ln_fwd_y16(n, d, _p(yb), _p(f["x"]), _p(f["gamma"]), _p(f["beta"]), b["eps"], p,
                                                _p(seed), R.MASK_OFFSET, _p(out), _p(mean), _p(rstd), None)
                    assert rc == 0
                    torch.cuda.synchronize()
                    what = (d, n, p, ld, "x16" if x16 else "y16")
                    assert _same(out, f["out"]) and _same(mean, f["mean"]) and _same(rstd, f["rstd"]), what
                for variant in ("dy16", "dy16_y16", "x16"):
                    dy, dx, part = _nan((n, ld), dtype=torch.bfloat16), _nan((n, d)), _nan((nb, 3, d))
                    if variant == "x16":
                        rc = lib.hsg_ln_bwd_x16(n, d, _p(dout), _p(yb), _p(xb), ld, _p(f["gamma"]), _p(f["mean"]),
                                                _p(f["rstd"]), p, _p(seed), R.MASK_OFFSET, _p(dy), ld, _p(dx),
                                                _p(part), None)
                    else:
                        y16 = variant == "dy16_y16"
                        rc = lib.hsg_ln_bwd_dy16(n, d, _p(dout), _p(yb if y16 else f["y"]), int(y16), _p(f["x"]),
                                                 _p(f["gamma"]), _p(f["mean"]), _p(f["rstd"]), p, _p(seed),
                                                 R.MASK_OFFSET, _p(dy), ld, _p(dx), _p(part), None)
                    assert rc == 0
                    torch.cuda.synchronize()
                    what = (d, n, p, ld, variant)
                    assert _same(dx, g["dx"]) and _same(part, g["part"][0]), what
                    assert _same(dy[:, :d], g["dy"].bfloat16()), what
                    assert not _bits(dy[:, d:ld0]).any(), what
                    assert torch.isnan(dy[:, ld0:]).all(), what


# ------------------------------------------------------------------ containment, determinism
FAMILY_WIDTHS = [(130, True), (300, False), (100, True), (300, True)]     # every forward and backward family


@pytest.mark.parametrize("d,aligned", FAMILY_WIDTHS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_element_stays_in_its_row(d, aligned, bad):
    n, r = 9, 5
    b = R.make_batch(d, n, "normal", 0.1, G=1)
    f0 = run_fwd(b, not aligned)
    g0 = run_bwd(b, f0, not aligned)
    b["x"][r, d // 3] = bad
    f1 = run_fwd(b, not aligned)
    g1 = run_bwd(b, f1, not aligned)
    others = [i for i in range(n) if i != r]
    for k in ("out", "mean", "rstd"):
        assert _same(f0[k][others], f1[k][others]), k
    assert torch.isnan(f1["out"][r]).all()
    for k in ("dx", "dy"):
        assert _same(g0[k][others], g1[k][others]), k
    keep = b["keep"][r].to(DEV)
    assert torch.isnan(g1["dx"][r]).all()
    assert torch.isnan(g1["dy"][r][keep]).all() and not g1["dy"][r][~keep].any()


@pytest.mark.parametrize("d,aligned", FAMILY_WIDTHS)
def test_two_runs_are_bitwise_equal(d, aligned):
    b = R.make_batch(d, 37, "normal", 0.1, G=1)
    runs = []
    for _ in range(2):
        f = run_fwd(b, not aligned)
        runs.append((f, run_bwd(b, f, not aligned)))
    (f0, g0), (f1, g1) = runs
    for k in ("out", "mean", "rstd"):
        assert _same(f0[k], f1[k]), k
    for k in ("dx", "dy", "part", "sums"):
        assert _same(g0[k], g1[k]), k


# ------------------------------------------------------------------ refusals (nothing is launched)
def test_refusals():
    from hetersumgraph_amd._lib import HSG_EINVAL
    lib = _lib()
    n, d = 8, 300
    z = lambda *s: torch.zeros(*s, device=DEV)
    y, x, g, out, mean, rstd, part = z(n, 520), z(n, 520), z(520), z(n, 520), z(n), z(n), z(2, 3, 520)
    dy, dx = z(n, 520), z(n, 520)
    seed = torch.tensor([1], dtype=torch.int64, device=DEV)

    def fwd(d=d, p=0.0, seed=None):
        return lib.hsg_ln_fwd(n, d, _p(y), _p(x), _p(g), _p(g), 1e-5, p, _p(seed), 0, _p(out), _p(mean), _p(rstd), None)

    def bwd(d=d, p=0.0, seed=None, part=part):
        return lib.hsg_ln_bwd(n, d, _p(out), _p(y), _p(x), _p(g), _p(mean), _p(rstd), p, _p(seed), 0, _p(dy), _p(dx),
                              _p(part), None)

    for call in (fwd, bwd):
        assert call(d=0) == HSG_EINVAL and call(d=513) == HSG_EINVAL
        assert call(p=1.0, seed=seed) == HSG_EINVAL and call(p=-0.1, seed=seed) == HSG_EINVAL
        assert call(p=0.1, seed=None) == HSG_EINVAL
    assert bwd(part=None) == HSG_EINVAL
    assert fwd() == 0 and bwd() == 0 and fwd(p=0.1, seed=seed) == 0
    torch.cuda.synchronize()

    yb = torch.zeros(n, 520, dtype=torch.bfloat16, device=DEV)
    xb = torch.zeros(n, 528, dtype=torch.bfloat16, device=DEV)
    dyb = torch.zeros(n, 528, dtype=torch.bfloat16, device=DEV)

    def f_y16(d=d, x=x):
        return lib.hsg_ln_fwd_y16(n, d, _p(yb), _p(x), _p(g), _p(g), 1e-5, 0.0, None, 0, _p(out), _p(mean), _p(rstd),
                                  None)

    def f_x16(d=d, xb=xb, ldx=304):
        return lib.hsg_ln_fwd_x16(n, d, _p(yb), _p(xb), ldx, _p(g), _p(g), 1e-5, 0.0, None, 0, _p(out), _p(mean),
                                  _p(rstd), None)

    def b_dy16(d=d, x=x, ld=304):
        return lib.hsg_ln_bwd_dy16(n, d, _p(out), _p(y), 0, _p(x), _p(g), _p(mean), _p(rstd), 0.0, None, 0, _p(dyb),
                                   ld, _p(z(n, 520)), _p(part), None)

    def b_x16(d=d, xb=xb, ldx=304, ld=304):
        return lib.hsg_ln_bwd_x16(n, d, _p(out), _p(yb), _p(xb), ldx, _p(g), _p(mean), _p(rstd), 0.0, None, 0,
                                  _p(dyb), ld, _p(z(n, 520)), _p(part), None)

    for call in (f_y16, f_x16, b_dy16, b_x16):
        assert call() == 0
        for bad in (256, 516, 302):                            # the vector kernels' widths only
            assert call(d=bad) == HSG_EINVAL, (call.__name__, bad)
    # a pointer off its alignment is refused by the host code before any launch
    assert f_y16(x=x.view(-1)[1:]) == HSG_EINVAL and b_dy16(x=x.view(-1)[1:]) == HSG_EINVAL
    assert f_x16(xb=xb.view(-1)[2:]) == HSG_EINVAL and b_x16(xb=xb.view(-1)[2:]) == HSG_EINVAL
    for ld in (300, 302, 296):                                 # pitch not a multiple of 8, or below ceil8(d)
        assert f_x16(ldx=ld) == HSG_EINVAL and b_x16(ldx=ld) == HSG_EINVAL
        assert b_dy16(ld=ld) == HSG_EINVAL and b_x16(ld=ld) == HSG_EINVAL
    torch.cuda.synchronize()
