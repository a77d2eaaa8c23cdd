"""The bound tests/test_gpu_rows.py holds the row kernels to is fair for exactly its
inputs, shown without a GPU: rows_ref's numpy fp32 restatement of the kernels' summation
order (lane- or quad-strided partial sums, the xor butterfly, fmaf variance, per-wave
column partials) stays within FACTOR = 4 times yard = max |fp32 CPU - fp64| of
torch.native_layer_norm on every (width, regime) the GPU test runs, and within the
analytic bound on rows of equal elements.  yard is positive for out, mean and rstd of every
(width, regime) except rows of equal elements -- the constant regime, and every row at d = 1
-- where torch's fp32 output is exact.  Also pins the family table's coverage."""
import numpy as np
import pytest
import torch

import rows_ref as R

N_CPU = 37                     # the largest of the GPU test's small row counts: 10 blocks, ragged


def _err(a, ref):
    return np.abs(np.asarray(a, np.float64) - ref.numpy()).max()


def _check_constant_forward(b, f, r64, what):
    bm, bo, rs0, rs_rel = R.constant_bounds(b)
    if b["d"] > 1:
        assert (np.abs(f["mean"].astype(np.float64) - r64["mean"].numpy()) <= bm.numpy()).all(), what
    assert (np.abs(f["out"].astype(np.float64) - r64["out"].numpy()) <= bo.numpy()).all(), what
    assert (np.abs(f["rstd"].astype(np.float64) / rs0 - 1) <= rs_rel).all(), what


@pytest.mark.parametrize("d,aligned", R.WIDTH_CASES)
def test_restated_order_within_the_bound(d, aligned):
    fwd, bwd = R.family("fwd", d, aligned), R.family("bwd", d, aligned)
    worst = {}
    for regime, p, eps, col in R.REGIMES:
        b = R.make_batch(d, N_CPU, regime, p, eps, col)
        r64, yard = R.references(b)
        what = (d, regime, p, eps, col)
        f = R.restated_fwd(b, R.order_of(fwd))
        if R.constant_rows(b):
            assert yard["out"] == 0, what                                  # torch's fp32 is exact there
            if d == 1:
                assert _err(f["mean"], r64["mean"]) <= R.FACTOR * yard["mean"], what
            else:
                assert yard["mean"] == 0, what
            _check_constant_forward(b, f, r64, what)
        else:
            for k in ("out", "mean", "rstd"):
                e = _err(f[k], r64[k])
                assert yard[k] > 0 and e <= R.FACTOR * yard[k], (what, k, e, yard[k])
                worst[k] = max(worst.get(k, 0.0), e / yard[k])
            if regime == "normal":
                assert _err(f["out"], r64["out"]) <= R.OUT_ABS, what
        g = R.restated_bwd(b, R.order_of(bwd), f["mean"], f["rstd"])
        sums = np.stack([R.restated_colsums(P.reshape(-1, 3 * d)).reshape(3, d) for P in g["part"]], 1)
        got = dict(dx=g["dx"], dy=g["dy"], dgamma=sums[0], dbeta=sums[1], db2=sums[2])
        for k in ("dx", "dy", "dgamma", "dbeta", "db2"):
            if k == "dgamma" and regime in R.DGAMMA_UNCHECKED:
                assert np.isfinite(got[k]).all(), what
                continue
            e = _err(got[k], r64[k])
            assert e <= R.FACTOR * yard[k], (what, k, e, yard[k])
            if yard[k] > 0:
                worst[k] = max(worst.get(k, 0.0), e / yard[k])
    print(f"d {d} {fwd} {bwd}: worst ratio " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_family_table_covers_every_family():
    fams = {(e, R.family(e, d, a)) for d, a in R.WIDTH_CASES for e in ("fwd", "bwd")}
    want = ({("fwd", f"fwd_scalar<{k}>") for k in range(1, 9)} | {("bwd", f"bwd_scalar<{k}>") for k in range(1, 9)} |
            {("fwd", "fwd_vec<1,2>"), ("fwd", "fwd_persistent<2,1>"), ("bwd", "bwd_vec<2>")})
    assert fams == want
    assert {R.family("fwd", d, True) for d in R.SCALAR_WIDTHS} == {f"fwd_scalar<{k}>" for k in range(1, 9)}
    assert {R.family("bwd", d, True) for d in R.SCALAR_WIDTHS} == {f"bwd_scalar<{k}>" for k in range(1, 9)}
    # a misaligned pointer sends the vector widths to the scalar kernels
    assert R.family("fwd", 64, False) == "fwd_scalar<1>" and R.family("fwd", 300, False) == "fwd_scalar<5>"
    assert R.family("bwd", 64, True) == "bwd_scalar<1>" and R.family("bwd", 300, False) == "bwd_scalar<5>"
    for d in R.VEC_WIDTHS:
        assert R.family("fwd", d, True) == "fwd_vec<1,2>" and R.family("bwd", d, True).startswith("bwd_scalar")
    for d in R.PERSISTENT_WIDTHS:
        assert R.family("fwd", d, True) == "fwd_persistent<2,1>" and R.family("bwd", d, True) == "bwd_vec<2>"


def test_every_regime_reaches_every_family_with_signed_gamma():
    """gamma holds zeros and negative entries at every width from 7 up, so in every family."""
    for d, _ in R.WIDTH_CASES:
        g = R.make_batch(d, 1)["gamma"]
        if d >= 7:
            assert (g == 0).any() and (g < 0).any() and (g > 0).any()


def test_wrap_cases_cross_each_grid():
    assert any(n > 32768 and R.family("fwd", d, True).startswith("fwd_scalar") for n, d in R.FWD_WRAPS)
    assert any(n > 6144 and R.family("fwd", d, True) == "fwd_persistent<2,1>" for n, d in R.FWD_WRAPS)
    for fam in ("bwd_scalar<1>", "bwd_scalar<3>", "bwd_vec<2>"):
        ns = sorted(n for n, d in R.BWD_WRAPS if R.family("bwd", d, True) == fam)
        assert ns[0] < 2048 < ns[-1] and 2048 in ns and R.bwd_blocks(ns[-1]) == 512


def test_restated_colsums_against_fp64():
    rng = np.random.default_rng(5)
    for rows in (1, 7, 8, 9, 31, 32, 33, 57, 512):
        P = rng.standard_normal((rows, 37)).astype(np.float32)
        ref = P.astype(np.float64).sum(0)
        yard = np.abs(R.seq_colsum32(P) - ref).max()
        assert np.abs(R.restated_colsums(P) - ref).max() <= R.FACTOR * yard, rows
