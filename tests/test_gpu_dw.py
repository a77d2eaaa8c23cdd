"""k_dw of csrc/hsg_dw.hip through the C ABI (hsg_gemm_dw_slabs, hsg_gemm_dw_slabs_io; the
product library) against fp64, slab by slab: every tile shape at ragged, exact and
multi-tile sizes, every K-slice plan, one and two jobs per launch, strides and K tails,
bf16 operands, the limb probes, five numeric regimes, containment of a non-finite element,
determinism, the product's own path (dense.gemm_dw_slabs + reduce.SlabBatch) and the dev
library's k_dw2.  Cases, references and the tolerance rule are tests/dw_ref.py's;
tests/test_dw_cpu.py shows on the CPU that the kernel's order of operations meets them.

Every workspace is NaN before the launch and carries one more slab of NaN behind the last:
after the launch every element of every slab is finite and that slab is still NaN (launch()).
Operand buffers hold NaN in their pad columns and in the rows from K up to the next
multiple of 32 throughout.

Tolerances: bitwise for the probes and the stated equalities; per slab
max err / unit <= 4 * max yard / unit for the dense cases (dw_ref: yard is the CPU's
sequential fp32 accumulation against fp64, never taken from the kernel).

Mutations these cases catch, each tried on a scratch copy of hsg_dw.hip (none is committed),
with the first case that fails (in file order) and the limb probes that see it:
  * each of the six MFMA lines of dw_tile removed in turn: test_shape_sweep[0-shape0-0] (the
    dense bound at (132, 124), K = 100, f32) for every one of them, and bitwise in
    test_limb_probes: a2b0 -- pair 2 alone; a1b1 -- pair 1 alone; a0b2 -- pair 3 alone; a1b0
    -- pairs 1 and 2; a0b1 -- pairs 1 and 3 (all f32 mode, all three tile kinds); a0b0 --
    every pair in both modes.  The 2e-6 bound of test_dw_slabs_pair passes the first five;
  * ``wn * WN`` written as ``wn * WM`` in dw_tile's epilogue: every 160 x 128 and 128 x 160
    shape of test_shape_sweep in both modes, first [0-shape0-0] (columns 64 .. 79 of the
    tile stay NaN), and every probe on those two kinds; the 128 x 128 shapes pass (WM = WN);
  * ``min(x, rem)`` written as ``x`` in xcd_order: test_shape_sweep[0-shape2-0] at splits = 2
    ((316, 260): 12 blocks, the first launch of the file with 8 or more) -- two logical blocks
    are never run (NaN left in slab 1) and two land in the NaN slab behind the last.  Any
    grid of 8 or more blocks whose count is not 7 mod 8 shows it, multiples of 8 included
    (test_dw_cpu.py); tried on that one case only, since further out the stray blocks leave
    the workspace;
  * job 1's ``start`` advanced without ``* splits``: test_two_jobs_equal_each_alone
    [a3-b3-2-0] ((484, 128) + (316, 260), splits 2: job 0's slab 1 is never written), and
    the two pairs with four slices;
  * the slab offset ``tz * M * N`` taken with the other job's M (when there are two jobs):
    the same three cases, first [a3-b3-2-0];
  * k_dw2 (dev library) with its a2b0 line removed: test_dw2_limb_probes[shape0-0] and
    test_dw2_k_slicing_equals_k_dw[shape0-0] -- so HSG_DW_V2=1 does reach k_dw2 there.
"""
import ctypes

import numpy as np
import pytest
import torch

import dw_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, VP = ctypes.c_int, ctypes.c_void_p
NAN = float("nan")


def _lib():
    from hetersumgraph_amd._lib import load
    return load()


def _einval():
    from hetersumgraph_amd._lib import HSG_EINVAL
    return HSG_EINVAL


def _arr(t, xs):
    return (t * len(xs))(*xs)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _operand(T, ld=None, bf=False):
    """Device rows of pitch ld for a CPU [K, cols] fp32 operand, as fp32 or bf16: ceil32(K) rows,
    NaN in every pad column and every row from K on -- allocated, never to be read."""
    K, c = T.shape
    buf = torch.full((-(-K // 32) * 32, ld or c), NAN, dtype=torch.bfloat16 if bf else torch.float32, device=DEV)
    buf[:K, :c] = T.to(DEV).to(buf.dtype)
    return buf


def _workspaces(jobs, splits):
    return [torch.full((splits + 1, A.shape[1], B.shape[1]), NAN, device=DEV) for A, B in jobs]


def _call(jobs, K, splits, bf16, io, As, Bs, Ws, lda=None, ldb=None, njobs=None, M=None, N=None, a_off=0, b_off=0):
    lib = _lib()
    n = len(jobs) if njobs is None else njobs
    args = [n, _arr(I32, M or [A.shape[1] for A, _ in jobs]), _arr(I32, N or [B.shape[1] for _, B in jobs]), K,
            _arr(VP, [a.data_ptr() + a_off for a in As]), _arr(I32, lda or [a.stride(0) for a in As]),
            _arr(VP, [b.data_ptr() + b_off for b in Bs]), _arr(I32, ldb or [b.stride(0) for b in Bs])]
    ws = _arr(VP, [w.data_ptr() for w in Ws])
    if io is not None:
        assert bf16
        return lib.hsg_gemm_dw_slabs_io(*args, _arr(I32, io), splits, ws, None)
    return lib.hsg_gemm_dw_slabs(*args, splits, int(bf16), ws, None)


def launch(jobs, splits, bf16, io=None, pads=None, finite=True):
    """One launch of jobs [(A [K, M], B [K, N])] (CPU fp32 tensors).  io: per-job operand bits
    (bit 0: A is bf16 rows, bit 1: B), through hsg_gemm_dw_slabs_io; pads: per-job (extra
    columns of A's pitch, of B's).  Returns each job's slabs [splits, M, N] on the CPU."""
    K = jobs[0][0].shape[0]
    pads = pads or [(0, 0)] * len(jobs)
    bits = io or [0] * len(jobs)
    As = [_operand(A, A.shape[1] + p[0], bool(i & 1)) for (A, _), p, i in zip(jobs, pads, bits)]
    Bs = [_operand(B, B.shape[1] + p[1], bool(i & 2)) for (_, B), p, i in zip(jobs, pads, bits)]
    Ws = _workspaces(jobs, splits)
    rc = _call(jobs, K, splits, bf16, io, As, Bs, Ws)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = []
    for q, w in enumerate(Ws):
        w = w.cpu()
        what = (q, tuple(w.shape), K, splits, bf16, io)
        assert torch.isnan(w[splits]).all(), ("the slab behind the last was written", what)
        if finite:
            assert torch.isfinite(w[:splits]).all(), ("an element was not written, or is not finite", what)
        out.append(w[:splits].clone())
    return out


def refused(jobs, splits, bf16, io=None, **kw):
    """The entry returns HSG_EINVAL and no workspace changes."""
    K = kw.pop("K", jobs[0][0].shape[0])
    bits = io or [0] * len(jobs)
    As = [_operand(A, None, bool(i & 1)) for (A, _), i in zip(jobs, bits)]
    Bs = [_operand(B, None, bool(i & 2)) for (_, B), i in zip(jobs, bits)]
    Ws = _workspaces(jobs, max(splits, 1))
    rc = _call(jobs, K, splits, bf16, io, As, Bs, Ws, **kw)
    torch.cuda.synchronize()
    return rc == _einval() and all(torch.isnan(w).all().item() for w in Ws)


class Worst:
    """The worst err / yard of the slabs behind one printed line."""

    def __init__(self):
        self.w = (-1.0, 0.0, 0.0)

    def add(self, err, yard):
        r = err / yard if yard > 0 else 0.0
        if r >= self.w[0]:
            self.w = (r, err, yard)

    def line(self, head):
        print(f"{head}: err {self.w[1]:.3e} yard {self.w[2]:.3e} ratio {self.w[0]:.2f}")


def check_dense(got, ref, unit, yard, worst, what):
    err, yd = D.ratios(got.numpy(), ref, unit, yard)
    for z in range(len(err)):
        worst.add(err[z], yd[z])
        assert err[z] <= D.FACTOR * yd[z], (what, "slab", z, err[z], yd[z])


def mode_name(bf16):
    return "bf16" if bf16 else "f32"


# ------------------------------------------------------------------ 1. shape sweep, one job
@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("cfg,shape", D.SHAPES)
def test_shape_sweep(cfg, shape, bf16):
    M, N = shape
    worst = Worst()
    for s in D.valid_splits(D.SWEEP_K):
        A, B, ref, unit, yard = D.dense_case(M, N, D.SWEEP_K, s, "normal", bf16)
        got, = launch([(A, B)], s, bf16)
        check_dense(got, ref, unit, yard, worst, (shape, s, bf16))
    worst.line(f"k_dw {D.KINDS[cfg]} sweep {M}x{N} K {D.SWEEP_K} {mode_name(bf16)}")


# ------------------------------------------------------------------ 2. K slicing and refusals
@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("K", D.SLICE_KS)
def test_k_slicing(K, bf16):
    for cfg, (M, N) in enumerate(D.RAGGED):
        worst = Worst()
        valid = D.valid_splits(K, D.SLICE_SPLITS_MAX)
        for s in valid:
            A, B, ref, unit, yard = D.dense_case(M, N, K, s, "normal", bf16)
            got, = launch([(A, B)], s, bf16)
            check_dense(got, ref, unit, yard, worst, ((M, N), K, s, bf16))
        A, B = D.dense_inputs(M, N, K, "normal")
        for s in range(0, D.k_tiles(K) + 3):
            if s not in valid and (s <= D.SLICE_SPLITS_MAX or s > D.k_tiles(K)):
                assert D.slice_plan(K, s) is None
                assert refused([(A, B)], s, bf16), (K, s)
        worst.line(f"k_dw {D.KINDS[cfg]} K {K} splits {valid} {mode_name(bf16)}")


def test_nine_k_tiles_refuse_four_slices():
    A, B = D.dense_inputs(132, 124, 257, "normal")
    for s in (4, 6, 7, 8, 10):
        assert refused([(A, B)], s, 0), s


def test_parameter_refusals():
    M, N = 132, 124
    A, B = D.dense_inputs(M, N, 64, "normal")
    j = [(A, B)]
    assert refused(j, 1, 0, M=[M - 2]) and refused(j, 1, 0, N=[N - 2])                 # M, N not a multiple of 4
    assert refused(j, 1, 0, lda=[M + 2]) and refused(j, 1, 0, ldb=[N + 2])             # pitches likewise
    assert refused(j, 1, 0, lda=[M - 4]) and refused(j, 1, 0, ldb=[N - 4])             # ... or below the width
    assert refused(j, 1, 0, a_off=4) and refused(j, 1, 0, b_off=8)                     # pointers off 16 bytes
    assert refused(j, 1, 1, io=[1], a_off=8) and refused(j, 1, 1, io=[2], b_off=8)
    assert refused(j, 1, 0, njobs=0) and refused(j + j, 1, 0, njobs=3)
    assert refused(j, 1, 1, io=[4]) and refused(j, 1, 1, io=[-1]) and refused(j + j, 1, 1, io=[0, 8])
    assert refused(j, 1, 0, K=0)
    got, = launch(j, 1, 0)                                                             # and the same job is accepted
    assert got.shape == (1, M, N)


# ------------------------------------------------------------------ 3. two jobs
@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("a,b,splits", D.PAIRS)
def test_two_jobs_equal_each_alone(a, b, splits, bf16):
    jobs = [D.dense_case(M, N, D.SWEEP_K, splits, "normal", bf16)[:2] for M, N in (a, b)]
    both = launch(jobs, splits, bf16)
    for q in range(2):
        alone, = launch([jobs[q]], splits, bf16)
        assert _same(both[q], alone), (a, b, splits, bf16, "job", q)


# ------------------------------------------------------------------ 4. strides and tails
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", D.RAGGED)
def test_strides_and_tails(shape, bf):
    """Pitches M + 4 / M + 8 and N + 4 / N + 8 on fp32 operands (both modes) and on bf16
    operands: NaN pads and NaN tail rows are never read."""
    M, N = shape
    A, B = D.dense_inputs(M, N, D.SWEEP_K, "normal")
    for bf16, io in (((1, [3]),) if bf else ((0, None), (1, None))):
        base, = launch([(A, B)], 2, bf16, io)
        for pa in (0, 4, 8):
            for pb in (0, 4, 8):
                got, = launch([(A, B)], 2, bf16, io, pads=[(pa, pb)])
                assert _same(got, base), (shape, bf16, io, pa, pb)


# ------------------------------------------------------------------ 5. bf16 operands
@pytest.mark.parametrize("shape", D.RAGGED)
def test_bf16_operands_bitwise(shape):
    """io = 0 .. 3 against hsg_gemm_dw_slabs(bf16 = 1) on the fp32 copies of the same values.
    The contiguous bf16 pitches 132 and 124 are multiples of 4 but not of 8."""
    M, N = shape
    assert (M % 8 == 4 or N % 8 == 4) and D.SWEEP_K % 32
    A, B = D.dense_inputs(M, N, D.SWEEP_K, "normal")
    for io in range(4):
        Av, Bv = (D.bf16_round(A) if io & 1 else A), (D.bf16_round(B) if io & 2 else B)
        want, = launch([(Av, Bv)], 2, 1)
        for pads in ((0, 0), (4, 8)):
            got, = launch([(Av, Bv)], 2, 1, io=[io], pads=[pads])
            assert _same(got, want), (shape, io, pads)
    # two jobs of different operand kinds in one launch
    A2, B2 = D.dense_inputs(N, M, D.SWEEP_K, "normal")
    Av, B2v = D.bf16_round(A), D.bf16_round(B2)
    want = launch([(Av, B), (A2, B2v)], 2, 1)
    got = launch([(Av, B), (A2, B2v)], 2, 1, io=[1, 2])
    assert _same(got[0], want[0]) and _same(got[1], want[1])


# ------------------------------------------------------------------ 6. limb probes
def check_probe(M, N, K, s, pair, bf16):
    A, B = D.probe(M, N, K, s, pair)
    got, = launch([(A, B)], s, bf16)
    want = torch.from_numpy(D.probe_expected(M, N, K, s, pair, bf16).astype(np.float32))
    bad = (_bits(got) != _bits(want))
    assert not bad.any(), ((M, N), K, s, "pair", pair + 1, mode_name(bf16), int(bad.sum()), "elements differ; first",
                           got[bad][0].item(), "expected", want[bad][0].item())
    return got


@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("pair", range(3))
@pytest.mark.parametrize("shape", D.RAGGED)
def test_limb_probes(shape, pair, bf16):
    for s in D.PROBE_SPLITS:
        check_probe(*shape, D.PROBE_K, s, pair, bf16)


# ------------------------------------------------------------------ 7. dense regimes
@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("regime", D.REGIMES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_dense_regimes(shape, regime, bf16):
    M, N = shape
    worst = Worst()
    for K, s in D.DENSE_KS:
        A, B, ref, unit, yard = D.dense_case(M, N, K, s, regime, bf16)
        got, = launch([(A, B)], s, bf16)
        check_dense(got, ref, unit, yard, worst, (shape, K, s, regime, bf16))
    worst.line(f"k_dw {D.KINDS[D.pick_cfg(M, N)]} {regime} {mode_name(bf16)}")


@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_large_and_small_are_the_normal_result_scaled(shape, bf16):
    M, N = shape
    for K, s in D.DENSE_KS:
        base, = launch([D.dense_inputs(M, N, K, "normal")], s, bf16)
        for regime, p in (("large", 2 * D.SCALE_EXP), ("small", -2 * D.SCALE_EXP)):
            got, = launch([D.dense_inputs(M, N, K, regime)], s, bf16)
            assert _same(got, (base.double() * 2.0 ** p).float()), (shape, K, regime, bf16)


@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_a_non_finite_element_stays_in_its_row_and_column(shape, bf16):
    M, N = shape
    for K, s in D.DENSE_KS:
        A, B = D.dense_inputs(M, N, K, "normal")
        clean, = launch([(A, B)], s, bf16)
        sl = D.slices(K, s)
        (ka, za), (kb, zb) = (sl[0][1] - 1, 0), (sl[-1][0], s - 1)      # last row of slice 0, first of the last
        m, n = M - 1, N - 2                                           # in the ragged part of the last tile
        A, B = A.clone(), B.clone()
        A[ka, m], B[kb, n] = NAN, float("inf")
        bad, = launch([(A, B)], s, bf16, finite=False)
        hit = torch.zeros(s, M, N, dtype=torch.bool)
        hit[za, m, :] = True
        hit[zb, :, n] = True
        assert not torch.isfinite(bad[hit]).any(), (shape, K, bf16)
        assert torch.equal(_bits(bad)[~hit], _bits(clean)[~hit]), (shape, K, bf16)


# ------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("bf16", D.MODES)
def test_two_launches_are_bitwise_equal(bf16):
    a, b, s = D.PAIRS[3]
    jobs = [D.dense_inputs(M, N, D.SWEEP_K, "wide") for M, N in (a, b)]
    first, second = launch(jobs, s, bf16), launch(jobs, s, bf16)
    assert _same(first[0], second[0]) and _same(first[1], second[1])


# ------------------------------------------------------------------ 9. the product's own path
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("K", D.PATH_KS)
@pytest.mark.parametrize("shapes", [((132, 124),), ((132, 124), (124, 132)), ((316, 260), (164, 128))])
def test_product_path(shapes, K, dtype):
    """dense.gemm_dw_slabs with its default slice rule, the slabs summed by reduce.SlabBatch
    into a zeroed-by-the-kernel dw and onto a non-zero one, against fp64 over the whole K."""
    from hetersumgraph_amd.dense import gemm_dtype, gemm_dw_slabs
    from hetersumgraph_amd.reduce import SlabBatch
    bf16 = int(dtype == "bf16")
    s = D.default_splits(shapes, K)
    assert s >= 2
    cpu = [D.dense_inputs(M, N, K, "normal") for M, N in shapes]
    dev = [(A.to(DEV), B.to(DEV)) for A, B in cpu]
    worst = Worst()
    for acc in (False, True):
        with gemm_dtype(dtype):
            res = gemm_dw_slabs(dev)
        assert res is not None and [sp for _, sp in res] == [s] * len(shapes)
        batch, outs, dws = SlabBatch(), [], []
        for q, ((M, N), (ws, sp)) in enumerate(zip(shapes, res)):
            dw = torch.randn(M, N, generator=torch.Generator().manual_seed(K + q))
            out = dw.to(DEV).reshape(-1).contiguous() if acc else torch.full((M * N,), NAN, device=DEV)
            batch.add(q, out, M * N, M * N, 0, 1.0, acc, ws, sp)
            outs.append(out)
            dws.append(dw)
        batch.flush()
        torch.cuda.synchronize()
        for (M, N), (A, B), out, dw in zip(shapes, cpu, outs, dws):
            ref, unit, yard = D.reduced_refs(A, B, s, bf16, dw if acc else None)
            got = out.cpu().double().view(M, N).numpy()
            assert np.isfinite(got).all()
            e, y = (np.abs(got - ref) / unit).max(), (yard / unit).max()
            worst.add(e, y)
            assert e <= D.FACTOR * y, (shapes, (M, N), K, dtype, acc, e, y)
    worst.line(f"gemm_dw_slabs + SlabBatch {shapes} K {K} splits {s} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_product_path_declines_one_slice(dtype):
    from hetersumgraph_amd.dense import gemm_dtype, gemm_dw_slabs
    assert D.default_splits([(132, 124)], 128) < 2
    A, B = D.dense_inputs(132, 124, 128, "normal")
    with gemm_dtype(dtype):
        assert gemm_dw_slabs([(A.to(DEV), B.to(DEV))]) is None


# ------------------------------------------------------------------ 10. k_dw2 (dev library)
def _v2(monkeypatch, on):
    if on:
        monkeypatch.setenv("HSG_DW_V2", "1")
    else:
        monkeypatch.delenv("HSG_DW_V2", raising=False)


@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_dw2_limb_probes(monkeypatch, shape, bf16):
    """k_dw2 (HSG_DW_V2=1, dev library): the probes are exact, and every slab is bitwise
    k_dw's -- per output element both kernels issue the same MFMAs on the same fragments in
    the same order; only the staging (two images, loads two tiles ahead) differs."""
    from helpers import skip_unless_dev
    skip_unless_dev(False)
    for K, s in [(D.PROBE_K, s) for s in D.PROBE_SPLITS] + list(D.V2_SLICES):
        for pair in range(3):
            _v2(monkeypatch, True)
            got = check_probe(*shape, K, s, pair, bf16)
            _v2(monkeypatch, False)
            assert _same(got, check_probe(*shape, K, s, pair, bf16)), (shape, K, s, pair, bf16)


@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_dw2_k_slicing_equals_k_dw(monkeypatch, shape, bf16):
    """Slices of 1 .. 5 K tiles (dw_ref.V2_SLICES) and the K-slicing sweep, one job and two:
    bitwise k_dw's slabs in the same library with the variable unset."""
    from helpers import skip_unless_dev
    skip_unless_dev(False)
    M, N = shape
    plans = list(D.V2_SLICES) + [(K, s) for K in D.SLICE_KS for s in D.valid_splits(K, D.SLICE_SPLITS_MAX)]
    for K, s in plans:
        jobs = [D.dense_inputs(M, N, K, "normal"), D.dense_inputs(N, M, K, "wide")]
        for js in (jobs[:1], jobs):
            _v2(monkeypatch, True)
            got = launch(js, s, bf16)
            _v2(monkeypatch, False)
            want = launch(js, s, bf16)
            assert all(_same(g, w) for g, w in zip(got, want)), (shape, K, s, bf16, len(js))
