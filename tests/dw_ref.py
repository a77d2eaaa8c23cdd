"""The FFN weight-gradient kernel of csrc/hsg_dw.hip (k_dw behind hsg_gemm_dw_slabs and
hsg_gemm_dw_slabs_io, k_dw2 in the dev library) against plain references: host restatements
of the tile rule, the K-slice plan and xcd_order, the case tables, the fp64 / fp32
references of every K slice, a numpy restatement of the kernel's six limb products and the
limb probes.  Shared by tests/test_dw_cpu.py and tests/test_gpu_dw.py; imports neither the
library nor a GPU.

Operation (autograd of PositionwiseFeedForward, module/GATLayer.py:39-41 of the original
model: dW2 = dY^T H, dW1 = dH^T X): job q of a launch has A [K][M] and B [K][N], both
row-major over k, and writes slab z of ws [splits][M][N] = A[k0_z:k1_z]^T B[k0_z:k1_z], the
partial product of K slice z.  'f32' mode: both operands split into three RNE bf16 limbs,
six of the nine limb products per 32-deep K tile on the bf16 MFMA, in the order PRODUCTS.
'bf16' mode: the one product of the RNE-rounded operands.

Tolerance convention (tests/rows_ref.py): a slab may err by FACTOR = 4 times ``yard``, the
error of a plain fp32 accumulation over k in order on the CPU (seq32: no BLAS call, whose
blocking is unknown) against fp64 on the same slice, both relative to unit = sum_k |a_k b_k|:
    max_e err_e / unit_e <= 4 * max_e yard_e / unit_e      per slab.
In 'bf16' mode the fp64 product, unit and the yardstick are taken on the RNE-rounded
operands.  tests/test_dw_cpu.py shows that the restated kernel meets this on exactly the
GPU test's inputs under both orderings the MFMA's inner sum may have (one rounding per 32
products, one per product).

Limb probes: inputs whose every slab is exact in fp32 under any summation order, built so
that each of the six limb products carries bits the others do not (probe()).
"""
import functools

import numpy as np
import torch

F32 = np.float32
FACTOR = 4
KBK = 32                                           # kBK: K rows per tile, one 16x16x32 MFMA step
TILES = ((160, 128), (128, 160), (128, 128))       # kTileM / kTileN, by cfg
KINDS = ("160x128", "128x160", "128x128")
PRODUCTS = ("a2b0", "a1b1", "a0b2", "a1b0", "a0b1", "a0b0")     # dw_tile's MFMA lines, in order
MODES = (0, 1)                                     # the entry's bf16 flag: 0 'f32', 1 'bf16'


# ------------------------------------------------------------------ host restatements
def pick_cfg(M, N):
    """pick_cfg of hsg_dw.hip: the tile with the least padded output area, ties to the first."""
    best, area = 0, None
    for c, (bm, bn) in enumerate(TILES):
        a = -(-M // bm) * bm * (-(-N // bn)) * bn
        if area is None or a < area:
            best, area = c, a
    return best


def tile_grid(M, N):
    """(cfg, tiles_m, tiles_n) of one job."""
    c = pick_cfg(M, N)
    return c, -(-M // TILES[c][0]), -(-N // TILES[c][1])


def tile_count(M, N):
    """hsg_gemm_dw_tiles(M, N)."""
    _, tm, tn = tile_grid(M, N)
    return tm * tn


def k_tiles(K):
    return -(-K // KBK)


def slice_plan(K, splits):
    """ktps (K tiles per slice) of dw_slabs' host code, or None where it returns HSG_EINVAL:
    splits above the K tile count, or a count whose slice length ceil(kt / splits) leaves
    fewer non-empty slices than the caller sized its workspace for."""
    kt = k_tiles(K)
    if K < 1 or splits < 1 or splits > kt:
        return None
    ktps = -(-kt // splits)
    return ktps if -(-kt // ktps) == splits else None


def valid_splits(K, upto=None):
    return [s for s in range(1, (upto or k_tiles(K)) + 1) if slice_plan(K, s) is not None]


def slices(K, splits):
    """[(k0, k1)]: the rows of every K slice (dw_tile's kt0 / kt1, rows clipped at K)."""
    ktps = slice_plan(K, splits)
    assert ktps is not None, (K, splits)
    return [(z * ktps * KBK, min(K, (z + 1) * ktps * KBK)) for z in range(splits)]


def xcd_order(b, total, clamp=True):
    """xcd_order of hsg_dw.hip: workgroup b -> logical block.  clamp=False: the mutation
    that drops min(x, rem)."""
    x, j, per, rem = b & 7, b >> 3, total >> 3, total & 7
    return x * per + (min(x, rem) if clamp else x) + j


def launch_blocks(shapes, splits):
    """Blocks of one launch: sum over jobs of tiles x splits."""
    return sum(tile_count(M, N) for M, N in shapes) * splits


# ------------------------------------------------------------------ case tables
# per tile kind: one ragged tile, an exact tile, more than one tile along M and along N with
# a ragged last one (128 x 128 also: the smallest shape the entry accepts)
SHAPES = ((0, (132, 124)), (0, (160, 128)), (0, (316, 260)), (0, (480, 128)),
          (1, (124, 132)), (1, (128, 160)), (1, (324, 132)), (1, (164, 260)),
          (2, (4, 4)), (2, (128, 128)), (2, (164, 128)), (2, (128, 164)), (2, (484, 128)))
for _c, (_m, _n) in SHAPES:
    assert pick_cfg(_m, _n) == _c, ("the tile rule of hsg_dw.hip changed", _m, _n, pick_cfg(_m, _n), _c)
RAGGED = ((132, 124), (124, 132), (164, 128))      # one ragged shape per tile kind, by cfg
assert [pick_cfg(m, n) for m, n in RAGGED] == [0, 1, 2]
assert tile_grid(164, 128)[1] == 2                 # the 128 x 128 tile with more than one tile along M

SWEEP_K = 100                                      # 4 K tiles (the last of 4 rows): splits 1, 2, 4
SLICE_KS = (1, 31, 32, 33, 64, 65, 257, 1000)
SLICE_SPLITS_MAX = 9
# two jobs per launch: (shape of job 0, shape of job 1, splits) at K = SWEEP_K
PAIRS = (((480, 128), (164, 260), 1),              # kinds 0, 1: 7 blocks, fewer than 8
         ((324, 132), (316, 260), 1),              # 1, 0: 9 blocks
         ((132, 124), (164, 128), 1),              # 0, 2: 3
         ((484, 128), (316, 260), 2),              # 2, 0: 20
         ((124, 132), (484, 128), 1),              # 1, 2: 5
         ((128, 164), (164, 260), 1),              # 2, 1: 6
         ((4, 4), (128, 128), 1),                  # 2, 2: 2
         ((132, 124), (124, 132), 4),              # 0, 1: 8
         ((164, 128), (132, 124), 4))              # 2, 0: 12
PROBE_K = 257
PROBE_SPLITS = (1, 3, 9)
# k_dw2: K slices of 1 .. 5 tiles, with and without a ragged last tile, and a lone row
V2_SLICES = ((1, 1), (33, 1), (257, 9), (257, 5), (257, 3), (250, 2), (257, 2), (150, 1))
DENSE_KS = ((257, 3), (1000, 4))
REGIMES = ("normal", "wide", "cancelling")         # large / small: normal scaled by 2^40 / 2^-40
SCALE_EXP = 40
PATH_KS = (256, 1000)                              # the product's own path (dense.gemm_dw_slabs)


# ------------------------------------------------------------------ inputs
def bf16_round(t):
    """RNE to bf16, as fp32 values (torch's conversion: v_cvt_pk_bf16_f32's rounding)."""
    return t.bfloat16().float()


def dense_inputs(M, N, K, regime):
    """fp32 operands A [K, M], B [K, N] of one dense case.
      normal      standard normal
      wide        standard normal times exp(2 randn) per entry
      cancelling  rows k and k + 1 (k even) have equal A, and B opposite up to 1e-3 relative:
                  every pair of products nearly cancels, so unit is large against the result
      large       the normal draws times 2^40        small       times 2^-40"""
    g = torch.Generator().manual_seed(7919 * M + 104729 * N + 31 * K + (0 if regime in ("large", "small") else
                                                                       REGIMES.index(regime)))
    A, B = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    if regime == "wide":
        A, B = A * torch.exp(2 * torch.randn(K, M, generator=g)), B * torch.exp(2 * torch.randn(K, N, generator=g))
    elif regime == "cancelling":
        d = 1 + 1e-3 * torch.randn(K, N, generator=g)
        for k in range(1, K, 2):
            A[k], B[k] = A[k - 1], -B[k - 1] * d[k]
    elif regime == "large":
        A, B = A * 2.0 ** SCALE_EXP, B * 2.0 ** SCALE_EXP
    elif regime == "small":
        A, B = A * 2.0 ** -SCALE_EXP, B * 2.0 ** -SCALE_EXP
    else:
        assert regime == "normal", regime
    return A.float().contiguous(), B.float().contiguous()


# ------------------------------------------------------------------ references
def seq32(A, B):
    """The yardstick: acc = fl(acc + fl(a_k b_k)) over k in order, fp32 numpy, no BLAS."""
    acc = np.zeros((A.shape[1], B.shape[1]), F32)
    for k in range(A.shape[0]):
        acc = acc + A[k][:, None] * B[k][None, :]
    return acc


def slab_refs(A, B, splits, bf16):
    """Per K slice: (ref [S, M, N] fp64 product, unit [S, M, N] = sum_k |a_k b_k|,
    yard [S, M, N] = |seq32 - ref|), on the RNE-rounded operands in bf16 mode."""
    if bf16:
        A, B = bf16_round(A), bf16_round(B)
    a32, b32 = A.numpy(), B.numpy()
    a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
    ref, unit, yard = [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for k0, k1 in slices(A.shape[0], splits):
            r = a64[k0:k1].T @ b64[k0:k1]
            ref.append(r)
            unit.append(np.abs(a64[k0:k1]).T @ np.abs(b64[k0:k1]))
            yard.append(np.abs(seq32(a32[k0:k1], b32[k0:k1]).astype(np.float64) - r))
    return np.stack(ref), np.stack(unit), np.stack(yard)


def ratios(got, ref, unit, yard):
    """Per slab: (max err / unit, max yard / unit).  The bound is the first <= FACTOR x the second."""
    u = np.maximum(unit, 1e-300)
    err = np.abs(np.asarray(got, np.float64) - ref)
    S = ref.shape[0]
    return (err / u).reshape(S, -1).max(1), (yard / u).reshape(S, -1).max(1)


@functools.lru_cache(maxsize=None)
def dense_case(M, N, K, splits, regime, bf16):
    """(A, B, ref, unit, yard) of one dense case; computed once, shared, never changed."""
    A, B = dense_inputs(M, N, K, regime)
    return (A, B) + slab_refs(A, B, splits, bf16)


# ------------------------------------------------------------------ the kernel's order
def split3(t):
    """hsg_split3: x0 = RNE(x), x1 = RNE(x - x0), x2 = RNE(x - x0 - x1) (the differences are
    exact in fp32).  Returns three fp64 numpy arrays."""
    x0 = bf16_round(t)
    r = t - x0
    x1 = bf16_round(r)
    x2 = bf16_round(r - x1)
    return [x.numpy().astype(np.float64) for x in (x0, x1, x2)]


def restated(A, B, splits, bf16, drop=None, per_product=False):
    """k_dw's slabs [S, M, N] in fp32 numpy: per K slice an fp32 accumulator, per 32-deep K
    tile the six limb products in PRODUCTS order ('bf16' mode: a0b0 of the rounded
    operands alone), each one MFMA over the tile's rows.  The MFMA's inner order is not
    documented; the two extremes are restated: one rounding per 32 products (the tile's
    sum formed exactly, then added), and per_product: one rounding per product, k in order.
    drop: the one product left out (a five-MFMA kernel)."""
    K = A.shape[0]
    a, b = ([bf16_round(A).numpy().astype(np.float64)], [bf16_round(B).numpy().astype(np.float64)]) if bf16 else \
        (split3(A), split3(B))
    names = ("a0b0",) if bf16 else PRODUCTS
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for k0, k1 in slices(K, splits):
            acc = np.zeros((A.shape[1], B.shape[1]), F32)
            for r0 in range(k0, k1, KBK):
                r1 = min(r0 + KBK, k1)
                for name in names:
                    if name == drop:
                        continue
                    x, y = a[int(name[1])], b[int(name[3])]
                    if per_product:
                        for k in range(r0, r1):
                            acc = (acc.astype(np.float64) + x[k][:, None] * y[k][None, :]).astype(F32)
                    else:
                        acc = (acc.astype(np.float64) + x[r0:r1].T @ y[r0:r1]).astype(F32)
            out.append(acc)
    return np.stack(out)


# ------------------------------------------------------------------ limb probes
# (va, vb): pair 1 has limbs (1, 2^-8, 0) on both sides (1 + 2^-8 is a tie, RNE takes the
# even 1) and carries a0b0, a0b1, a1b0, a1b1; pairs 2 and 3 have (1, 2^-9, 2^-18) on one
# side and 1 on the other and add a2b0 / a0b2.  a1b2, a2b1 and a2b2 -- the products the
# kernel drops by design -- are zero in all three.
PROBE_PAIRS = ((1 + 2.0 ** -8, 1 + 2.0 ** -8), (1 + 2.0 ** -9 + 2.0 ** -18, 1.0), (1.0, 1 + 2.0 ** -9 + 2.0 ** -18))
PROBE_ROWS_MAX = 16


def probe_rows(K, splits):
    """Per K slice, the rows k that are not zero: its first and last row (the last slice's
    last row is K - 1), and rows 0, 7, 8 and 31 of one tile inside a slice -- the second
    tile of the first slice with three or more, else with two, else the first tile of slice
    0 (rows past the slice are left out).  A slab's value depends on its own rows only, and
    no slice holds more than PROBE_ROWS_MAX = 16 of them, which is what keeps every partial
    sum of a slab inside 23 bits; the launch as a whole holds more than 16 once it has nine
    slices (first and last row of each are 17 rows at K = 257, splits = 9)."""
    sl = slices(K, splits)
    rows = [{k0, k1 - 1} for k0, k1 in sl]
    tiles = [-(-(k1 - k0) // KBK) for k0, k1 in sl]
    z = next((i for i, t in enumerate(tiles) if t >= 3), next((i for i, t in enumerate(tiles) if t == 2), 0))
    t0 = sl[z][0] + (KBK if tiles[z] >= 2 else 0)
    rows[z] |= {t0 + r for r in (0, 7, 8, 31) if t0 + r < sl[z][1]}
    rows = [sorted(r) for r in rows]
    assert all(len(r) <= PROBE_ROWS_MAX for r in rows)
    return rows


def probe_exponents(M, N):
    """e(m), f(n): both cycle through -6 .. 6, with periods (13, and 13 walked in steps of 5)
    that no tile, wave or fragment width divides."""
    return (np.arange(M) % 13) - 6, (5 * np.arange(N)) % 13 - 6


def probe_signs(M, nrows):
    """s(j, m) for the j-th probe row of a slice with nrows of them: column m is negative
    where m % 3 == 0, and the second row is flipped when the slice has three or more.  The
    slab's count sum_j s(j, m) is then +-nrows or +-(nrows - 2): never zero, and of opposite
    sign on some neighbour of every column."""
    s = np.where(np.arange(M) % 3 == 0, -1.0, 1.0)[None, :].repeat(nrows, 0)
    if nrows >= 3:
        s[1] *= -1
    return s


def probe(M, N, K, splits, pair):
    """(A [K, M], B [K, N]) fp32: zero except at probe_rows, where
    A[k, m] = s(k, m) 2^e(m) va and B[k, n] = 2^f(n) vb."""
    va, vb = PROBE_PAIRS[pair]
    e, f = probe_exponents(M, N)
    A, B = np.zeros((K, M)), np.zeros((K, N))
    for rows in probe_rows(K, splits):
        s = probe_signs(M, len(rows))
        for j, k in enumerate(rows):
            A[k] = s[j] * 2.0 ** e * va
            B[k] = 2.0 ** f * vb
    A32, B32 = A.astype(F32), B.astype(F32)
    assert (A32 == A).all() and (B32 == B).all()
    return torch.from_numpy(A32), torch.from_numpy(B32)


def probe_expected(M, N, K, splits, pair, bf16):
    """The exact slabs [S, M, N] as fp64: the fp64 product in f32 mode (it fits fp32:
    tests/test_dw_cpu.py), count * scale in bf16 mode (va and vb round to 1)."""
    A, B = probe(M, N, K, splits, pair)
    if not bf16:
        a, b = A.numpy().astype(np.float64), B.numpy().astype(np.float64)
        return np.stack([a[k0:k1].T @ b[k0:k1] for k0, k1 in slices(K, splits)])
    e, f = probe_exponents(M, N)
    scale = 2.0 ** (e[:, None] + f[None, :])
    return np.stack([probe_signs(M, len(rows)).sum(0)[:, None] * scale for rows in probe_rows(K, splits)])


# ------------------------------------------------------------------ the product's own path
def default_splits(shapes, K):
    """dense.gemm_dw_slabs' default slice count (two blocks per CU over all pairs' tiles, at
    least 4 K tiles per slice, every slice non-empty); below 2 it returns None."""
    kt = k_tiles(K)
    tiles = sum(tile_count(M, N) for M, N in shapes)
    splits = max(1, min(max(1, (2 * 256) // max(tiles, 1)), kt // 4))
    per = -(-kt // splits)
    return -(-kt // per)


def reduced_refs(A, B, splits, bf16, dw=None):
    """The reduced gradient (+ dw when accumulating) over the whole K: (ref, unit, yard).
    The yardstick adds each slice's seq32 in index order onto dw (or zero) in fp32."""
    if bf16:
        A, B = bf16_round(A), bf16_round(B)
    a32, b32 = A.numpy(), B.numpy()
    a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
    ref, unit = a64.T @ b64, np.abs(a64).T @ np.abs(b64)
    acc = np.zeros(ref.shape, F32) if dw is None else dw.numpy().astype(F32).copy()
    for k0, k1 in slices(A.shape[0], splits):
        acc = acc + seq32(a32[k0:k1], b32[k0:k1])
    if dw is not None:
        ref, unit = ref + dw.numpy().astype(np.float64), unit + np.abs(dw.numpy().astype(np.float64))
    return ref, unit, np.abs(acc.astype(np.float64) - ref)
