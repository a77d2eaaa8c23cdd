"""k_gemm13 (hsg_gemm_f32_psw_plan, plan 13: 160 x 128 blocks of 80 x 64 wave tiles, or
192 x 128 of 96 x 64 where colsum_part's 64-row slabs are asked for) against
k_gemm7<64> (plan 7): the same fragments, products and summation order, so C and the
64-row column partials are bitwise equal -- over partial row and column tiles,
the K tail inside a 32-deep tile, a single K tile, several K tiles through the one
stage, odd row counts across the 2 x 2 wave split, every epilogue, with and without
colsum_part.  One fp64 comparison with test_gpu_gemm.py's bounds for hsg_gemm_f32_psw,
and the router's switch-over row count."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BMS = (160, 192)                                           # without / with colsum_part
MS = sorted({1, 63, 64, 65} | {m for BM in BMS for m in (BM - 1, BM, BM + 1, 2 * BM + 17)})
NS = [512, 508, 324]
KS = [4, 28, 32, 36, 300, 512]
EPIS = ["none", "bias_relu", "add", "relu_bwd"]
MMAX = max(MS)

_cache = {}


def operands(N, K):
    """Seeded normal operands for the largest M (smaller M are row prefixes); a few rows
    of A and of the weight scaled by 1e3 / 1e-3 so all three limbs carry weight."""
    if (N, K) not in _cache:
        from hetersumgraph_amd.dense import split_weights
        g = torch.Generator(device="cuda").manual_seed(1000 * N + K)
        A = torch.randn(MMAX, K, device="cuda", generator=g)
        W = torch.randn(N, K, device="cuda", generator=g)
        for t, n in ((A, MMAX), (W, N)):
            t[0::7] *= 1e3
            t[3::11] *= 1e-3
            t[n - 1] *= 1e3
        aux = torch.randn(MMAX, N, device="cuda", generator=g)
        bias = torch.randn(N, device="cuda", generator=g)
        (S,) = split_weights((W, False))
        _cache.clear()                                     # one (N, K) set alive at a time
        _cache[(N, K)] = (A, W, aux, bias, S)
    return _cache[(N, K)]


def run(plan, A, S, aux, bias, epi, colsum):
    from hetersumgraph_amd.dense import gemm_psw, psw_row_tiles
    M, K = A.shape
    part = torch.full((psw_row_tiles(M, S.N, K), S.N), -7.0, device="cuda") if colsum else None
    kw = {"bias_relu": dict(bias=bias, relu=True), "add": dict(add=aux), "relu_bwd": dict(relu_mask=aux),
          "none": {}}[epi]
    C = gemm_psw(A, S, colsum_part=part, plan=plan, **kw)
    return C, part


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_plan13_is_bitwise_plan7(N, K):
    A, _, aux, bias, S = operands(N, K)
    for M in MS:
        for epi in EPIS:
            for colsum in (False, True):
                C7, p7 = run(7, A[:M], S, aux[:M], bias, epi, colsum)
                C13, p13 = run(13, A[:M], S, aux[:M], bias, epi, colsum)
                assert torch.equal(C13, C7), (M, N, K, epi, colsum)
                if colsum:
                    assert p7.shape[0] == (M + 63) // 64
                    assert not (p7 == -7.0).all(1).any()                 # every slab written
                    assert torch.equal(p13, p7), (M, N, K, epi)


def test_plan13_against_fp64():
    """(2 BM + 17, 512, 300) for both block heights: test_gpu_gemm.py's two bounds for
    hsg_gemm_f32_psw -- the absolute one of test_psw_layouts on standard-normal operands, and the per-element
    bound of test_psw_split_is_fp32_class in units of sum_k |a_k b_k| on the scaled ones."""
    from hetersumgraph_amd.dense import gemm_psw, split_weights
    N, K = 512, 300
    for M in (2 * BMS[0] + 17, 2 * BMS[1] + 17):
        g = torch.Generator(device="cuda").manual_seed(13)
        A = torch.randn(M, K, device="cuda", generator=g)
        W = torch.randn(N, K, device="cuda", generator=g)
        (S,) = split_weights((W, False))
        err = (gemm_psw(A, S, plan=13).double() - A.double() @ W.double().t()).abs().max().item()
        print(f"plan 13 {M}x{N}x{K}: max abs err {err:.3e}")
        assert err <= 1e-5 * max(1.0, K ** 0.5) * 4, err
    A, W, _, _, S = operands(N, K)
    ref = A.double() @ W.double().t()
    unit = A.double().abs() @ W.double().abs().t()
    e = ((gemm_psw(A, S, plan=13).double() - ref).abs() / unit).max().item()
    print(f"plan 13 {MMAX}x{N}x{K}: max err / sum|a||b| {e:.3e}")
    assert e < 2e-6, e


def test_plan_rejects():
    from hetersumgraph_amd._lib import HSG_EINVAL, load
    lib = load()
    A = torch.randn(64, 32, device="cuda")
    planes = torch.zeros(3 * 128 * 32, dtype=torch.bfloat16, device="cuda")
    C = torch.empty(64, 64, device="cuda")
    args = (64, 64, 32, A.data_ptr(), 32, planes.data_ptr(), C.data_ptr(), 64, None, None, 0, 0, 0, None)
    assert lib.hsg_gemm_f32_psw_plan(*args, 5, None) == HSG_EINVAL          # no such plan
    C2 = torch.empty(64, 66, device="cuda")                                 # ldc % 4 != 0: no float4 rows
    bad = args[:6] + (C2.data_ptr(), 66) + args[8:]
    assert lib.hsg_gemm_f32_psw_plan(*bad, 13, None) == HSG_EINVAL
    assert lib.hsg_gemm_f32_psw_plan(*bad, 7, None) == HSG_EINVAL
    assert lib.hsg_gemm_f32_psw_plan(*args, 13, None) == 0
    torch.cuda.synchronize()


def test_router_switches_at_the_rule():
    """Plan 0 is plan 13 from the smallest M the row-count rule routes to it (N = 512:
    where k_gemm7<64> needs a third round of the resident slots and the 160 | 192 x 128
    tiles still fit one, with or without colsum_part) and plan 7 just below; the outputs
    agree bitwise on both sides."""
    from hetersumgraph_amd._lib import load
    from hetersumgraph_amd.dense import gemm_psw, split_weights
    lib = load()
    N, K = 512, 32
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.hsg_gemm_f32_psw_route(1, N, K) == 7
    assert lib.hsg_gemm_f32_psw_route(19200, 300, 512) == 7                 # N <= 320 keeps its kernel
    # k_gemm7's third round starts at 2 * slots / 8 row tiles of 128
    M = 128 * (2 * 2 * cus // 8) + 1
    assert lib.hsg_gemm_f32_psw_route(M - 1, N, K) == 7
    assert lib.hsg_gemm_f32_psw_route(M, N, K) == 13
    if cus == 256:
        assert lib.hsg_gemm_f32_psw_route(19200, N, 300) == 13              # the cfg2 FFN shape
    g = torch.Generator(device="cuda").manual_seed(7)
    A = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g)
    (S,) = split_weights((W, False))
    for m in (M - 1, M):
        for colsum in (False, True):
            parts = [torch.full(((m + 63) // 64, N), -7.0, device="cuda") if colsum else None for _ in range(3)]
            C0 = gemm_psw(A[:m], S, colsum_part=parts[0], plan=0)
            assert torch.equal(C0, gemm_psw(A[:m], S, colsum_part=parts[1], plan=13))
            assert torch.equal(C0, gemm_psw(A[:m], S, colsum_part=parts[2], plan=7))
            if colsum:
                assert torch.equal(parts[0], parts[1]) and torch.equal(parts[0], parts[2])
