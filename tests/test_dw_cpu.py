"""tests/dw_ref.py without a GPU: the host restatements against the library's host-only
query and against exhaustive arithmetic, the case tables' coverage, the limb probes'
exactness and their power to see each of the six limb products, and the fairness of the
4 x yard bound tests/test_gpu_dw.py holds k_dw to -- the restated kernel meets it per slab on
exactly that test's inputs, under both orderings the MFMA's inner sum may have."""
import numpy as np
import pytest

import dw_ref as D


# ------------------------------------------------------------------ host restatements
def test_xcd_order_is_a_bijection():
    for total in range(1, 601):
        assert sorted(D.xcd_order(b, total) for b in range(total)) == list(range(total)), total


def test_xcd_order_without_the_clamp_is_not():
    """The mutation test_gpu_dw.py names (x in place of min(x, rem)): from 8 blocks up, every
    total but those with a remainder of 7 leaves logical blocks unvisited and sends as many
    workgroups up to 6 blocks past the last one -- into the slab behind the job's last, which
    is one reason the GPU test's workspaces carry a NaN slab there."""
    for total in range(1, 601):
        hit = sorted(D.xcd_order(b, total, clamp=False) for b in range(total))
        assert (hit != list(range(total))) == (total >= 8 and total % 8 != 7), total
        assert hit[-1] <= total + 6
    assert any(D.launch_blocks([s], k) >= 8 for _, s in D.SHAPES for k in D.valid_splits(D.SWEEP_K))


def test_tile_count_equals_the_library():
    """hsg_gemm_dw_tiles is a host-only query (tests/test_abi.py): no GPU needed."""
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    shapes = [s for _, s in D.SHAPES] + [(m, n) for m in range(4, 700, 28) for n in range(4, 700, 44)]
    for m, n in shapes:
        assert D.tile_count(m, n) == lib.hsg_gemm_dw_tiles(m, n), (m, n)


def test_splits_rule_against_exhaustive_ceil_arithmetic():
    """splits is valid exactly when some slice length L (in K tiles) gives ``splits`` slices
    that are all non-empty, and the kernel's L = ceil(kt / splits) is then that length."""
    for K in range(1, 401):
        kt = -(-K // 32)
        for splits in range(1, kt + 3):
            # all (L, splits) with splits slices of L tiles covering kt, the last one non-empty
            lengths = [L for L in range(1, kt + 1) if (splits - 1) * L < kt <= splits * L]
            plan = D.slice_plan(K, splits)
            want = -(-kt // splits) if splits <= kt else None
            assert (plan is not None) == (want in lengths), (K, splits)
            if plan is not None:
                assert plan == want
                sl = D.slices(K, splits)
                assert sl[0][0] == 0 and sl[-1][1] == K and all(k0 < k1 for k0, k1 in sl)
                assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    assert D.slice_plan(257, 4) is None and D.slice_plan(257, 10) is None      # nine K tiles
    assert D.valid_splits(D.SWEEP_K) == [1, 2, 4]
    assert D.valid_splits(257, 9) == [1, 2, 3, 5, 9]


# ------------------------------------------------------------------ case tables
def test_shape_table_coverage():
    for c in range(3):
        bm, bn = D.TILES[c]
        grids = [(M, N, D.tile_grid(M, N)) for cc, (M, N) in D.SHAPES if cc == c]
        assert all(g[0] == c for _, _, g in grids)
        assert any(g[1:] == (1, 1) and (M % bm or N % bn) for M, N, g in grids)        # one ragged tile
        assert any(g[1:] == (1, 1) and (M, N) == (bm, bn) for M, N, g in grids)        # an exact tile
        assert any(g[1] > 1 and M % bm for M, N, g in grids)                           # ragged last tile along M
        assert any(g[2] > 1 and N % bn for M, N, g in grids)                           # ... along N
    assert all(M % 4 == 0 and N % 4 == 0 and M <= 512 and N <= 512 for _, (M, N) in D.SHAPES)


def test_pair_table_coverage():
    kinds = {(D.pick_cfg(*a), D.pick_cfg(*b)) for a, b, _ in D.PAIRS}
    assert {(i, j) for i in range(3) for j in range(3) if i != j} <= kinds
    blocks = [D.launch_blocks((a, b), s) for a, b, s in D.PAIRS]
    assert min(blocks) < 8 and {n % 8 for n in blocks} >= set(range(1, 8))
    assert all(D.slice_plan(D.SWEEP_K, s) for _, _, s in D.PAIRS)
    # a job whose slab is not the other's size, with more than one slab: the slab-offset mutation
    assert any(s > 1 and a[0] != b[0] for a, b, s in D.PAIRS)


def test_v2_slices_cover_one_to_five_tiles():
    per = {D.slice_plan(K, s) for K, s in D.V2_SLICES}
    assert per >= {1, 2, 3, 4, 5}
    assert {D.slice_plan(D.PROBE_K, s) for s in D.PROBE_SPLITS} == {9, 3, 1}


# ------------------------------------------------------------------ limb probes
PROBE_CASES = [(M, N, K, s) for M, N in D.RAGGED for K, s in [(D.PROBE_K, s) for s in D.PROBE_SPLITS] + list(D.V2_SLICES)]


def test_probe_limbs():
    import torch
    for (va, vb), want in zip(D.PROBE_PAIRS, (((1, 2.0 ** -8, 0), (1, 2.0 ** -8, 0)),
                                              ((1, 2.0 ** -9, 2.0 ** -18), (1, 0, 0)),
                                              ((1, 0, 0), (1, 2.0 ** -9, 2.0 ** -18)))):
        la = [float(x[0]) for x in D.split3(torch.tensor([va], dtype=torch.float32))]
        lb = [float(x[0]) for x in D.split3(torch.tensor([vb], dtype=torch.float32))]
        assert (tuple(la), tuple(lb)) == want
        assert la[1] * lb[2] == 0 and la[2] * lb[1] == 0 and la[2] * lb[2] == 0      # dropped by design


def test_probe_rows():
    for K, s in [(D.PROBE_K, s) for s in D.PROBE_SPLITS] + list(D.V2_SLICES):
        rows, sl = D.probe_rows(K, s), D.slices(K, s)
        for r, (k0, k1) in zip(rows, sl):
            assert r[0] == k0 and r[-1] == k1 - 1 and len(r) <= 16
        assert rows[-1][-1] == K - 1
    r = D.probe_rows(257, 3)[0]                    # slices of three tiles: rows 0, 7, 8, 31 of the middle one
    assert r == [0, 32, 39, 40, 63, 95]


@pytest.mark.parametrize("bf16", D.MODES)
def test_probes_are_exact_and_restated_bitwise(bf16):
    for M, N, K, s in PROBE_CASES:
        for pair in range(3):
            A, B = D.probe(M, N, K, s, pair)
            want = D.probe_expected(M, N, K, s, pair, bf16)
            assert (want != 0).all() and (want.astype(np.float32).astype(np.float64) == want).all()
            if bf16:                               # count * scale is the fp64 product of the rounded operands
                a, b = D.bf16_round(A).numpy().astype(np.float64), D.bf16_round(B).numpy().astype(np.float64)
                assert all((a[k0:k1].T @ b[k0:k1] == w).all() for (k0, k1), w in zip(D.slices(K, s), want))
            # neighbouring columns and rows differ
            assert (want[:, 1:] != want[:, :-1]).all() and (want[:, :, 1:] != want[:, :, :-1]).all()
            for per_product in (False, True):
                got = D.restated(A, B, s, bf16, per_product=per_product)
                assert (got.view(np.int32) == want.astype(np.float32).view(np.int32)).all(), (M, N, K, s, pair)


def test_each_dropped_product_moves_a_probe():
    M, N = D.RAGGED[0]
    for drop in D.PRODUCTS:
        moved = []
        for s in D.PROBE_SPLITS:
            for pair in range(3):
                A, B = D.probe(M, N, D.PROBE_K, s, pair)
                want = D.probe_expected(M, N, D.PROBE_K, s, pair, 0).astype(np.float32)
                got = D.restated(A, B, s, 0, drop=drop)
                moved.append(not (got.view(np.int32) == want.view(np.int32)).all())
                if moved[-1]:                      # and it moves every slab's every element
                    assert (got != want).all(), (drop, s, pair)
        assert any(moved), drop


# ------------------------------------------------------------------ the dense bound is attainable
@pytest.mark.parametrize("bf16", D.MODES)
@pytest.mark.parametrize("regime", D.REGIMES)
@pytest.mark.parametrize("shape", D.RAGGED)
def test_restated_kernel_within_the_bound(shape, regime, bf16):
    M, N = shape
    for K, s in D.DENSE_KS:
        A, B, ref, unit, yard = D.dense_case(M, N, K, s, regime, bf16)
        for per_product in (False, True):
            err, yd = D.ratios(D.restated(A, B, s, bf16, per_product=per_product), ref, unit, yard)
            print(f"{D.KINDS[D.pick_cfg(M, N)]} K {K} {regime} bf16 {bf16} per_product {per_product}: err/yard "
                  + " ".join(f"{e / y:.2f}" for e, y in zip(err, yd)))
            assert (yd > 0).all() and (err <= D.FACTOR * yd).all(), (shape, K, regime, bf16, per_product, err, yd)


def test_a_dropped_product_is_outside_the_bound_on_dense_inputs():
    """What the 2e-6 bound of test_dw_slabs_pair cannot see: a five-MFMA kernel moves the
    normal-regime result by more than 4 x yard (a1b1's 2^-18 |ab| is the smallest)."""
    M, N = D.RAGGED[0]
    K, s = D.DENSE_KS[0]
    A, B, ref, unit, yard = D.dense_case(M, N, K, s, "normal", 0)
    for drop in D.PRODUCTS:
        err, yd = D.ratios(D.restated(A, B, s, 0, drop=drop), ref, unit, yard)
        assert (err > D.FACTOR * yd).all(), (drop, err / yd)


def test_scaling_by_a_power_of_two_commutes_with_the_split():
    M, N = D.RAGGED[2]
    K, s = D.DENSE_KS[0]
    A, B = D.dense_inputs(M, N, K, "normal")
    base = D.restated(A, B, s, 0)
    for regime, p in (("large", 2 * D.SCALE_EXP), ("small", -2 * D.SCALE_EXP)):
        As, Bs = D.dense_inputs(M, N, K, regime)
        assert (As == A * 2.0 ** (p // 2)).all()
        got = D.restated(As, Bs, s, 0)
        assert ((base.astype(np.float64) * 2.0 ** p).astype(np.float32).view(np.int32) == got.view(np.int32)).all()


@pytest.mark.parametrize("bf16", D.MODES)
def test_reduced_gradient_of_the_restated_slabs_within_the_bound(bf16):
    """Case 9's bound: the restated slabs summed in index order, with and without a dw."""
    import torch
    M, N = D.RAGGED[0]
    for K in D.PATH_KS:
        s = D.default_splits([(M, N)], K)
        assert s >= 2
        A, B = D.dense_inputs(M, N, K, "normal")
        slabs = D.restated(A, B, s, bf16)
        dw = torch.randn(M, N, generator=torch.Generator().manual_seed(K))
        for acc in (None, dw):
            tot = np.zeros((M, N), np.float32) if acc is None else acc.numpy().copy()
            for z in range(s):
                tot = tot + slabs[z]
            ref, unit, yard = D.reduced_refs(A, B, s, bf16, acc)
            e, y = (np.abs(tot - ref) / unit).max(), (yard / unit).max()
            assert y > 0 and e <= D.FACTOR * y, (K, bf16, acc is not None, e / y)
    assert D.default_splits([(M, N)], 128) < 2
