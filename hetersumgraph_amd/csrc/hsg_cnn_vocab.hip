// hsg_cnn_vocab.hip -- the sentence CNN's inference forward on a vocabulary product table for
// gfx950.  C ABI and the value contract: include/hsg_cnn_vocab.h.
//
// TW = [E ; P] Wall^T is a constant of an evaluation pass, so the forward is a gather: every
// element of a sentence's TW rows is used exactly once (element q(h, i, c) of row r belongs to
// window t = r - i of height h).  k_vocab_pool, one block per sentence:
//   * the sentence's token numbers go to LDS once (an id outside [0, V) as PAD);
//   * a tile of kRows consecutive positions is read as WHOLE rows with 16-byte loads, two vectors
//     per thread and row -- the token row into registers one tile ahead, under the sums of the
//     tile before, the (cached) position row next to it -- and the sums a + p are written to LDS;
//   * wave p owns heights 2 + p and 7 - p (9 taps: the three waves carry equal work), lane c one
//     channel.  A window's partial sums move down a register chain, one tap per row:
//     w[i] = w[i - 1] + x(r)[q(h, i, c)], w[0] = b + x(r)[q(h, 0, c)], so after row r, w[h - 1] is
//     the finished window t = r - h + 1: exactly v = b; v = v + (a + p) in ascending i.  The chain
//     lives across tiles, so no row is staged twice;
//   * the rows past the sentence's end are the pad row, kept in registers (9 sums per lane).
// Windows finish in ascending t, so strict > keeps the first maximum.  Every barrier is in the
// kernel's one tile loop, whose trip count (len) is the block's; only the sums between two
// barriers branch on the wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_cnn_vocab.h"

// the value contract is written in separately rounded adds, as hsg_cnn_tokens.hip's (the file is
// also built with -ffp-contract=off, build.py FILE_FLAGS)
#pragma clang fp contract(off)

namespace {

constexpr int kGroups = 6;      // kernel heights 2..7
constexpr int kCh = 50;         // channels per height
constexpr int kTaps = 27;       // 2 + 3 + ... + 7
constexpr int kNY = kTaps * kCh;
constexpr int kFeat = kGroups * kCh;
constexpr int kMaxL = 400;
constexpr int kThreads = 192;   // three waves: heights (2,7), (3,6), (4,5)
constexpr int kRows = 5;        // positions per tile: 28 KB of LDS, five blocks per CU
constexpr int kRow4 = (kNY + 3) / 4;                         // 338 16-byte vectors cover a row
constexpr int kPitch = kRow4 * 4;                            // LDS row pitch in floats (1352)
constexpr int kPer = 2 * kRows;                              // vectors per thread and tile: two per row
static_assert(kRow4 <= 2 * kThreads, "a row is two vectors per thread");

__host__ __device__ constexpr int tap_base(int g) { return g * (g + 3) / 2; }   // sum_{j<g} (j+2)

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

__device__ inline int sent_len(const int32_t *__restrict__ rowoff, int s, int L) {
    int len = rowoff[s + 1] - rowoff[s] - 1;
    len = len < 0 ? 0 : len;
    return len > L ? L : len;
}

struct Bias {
    const float *b[kGroups];
};

// One row through the chain of height H, kept in w[K0 .. K0 + H - 1]: x[K0 + i] = the row's sum
// at tap i.
template <int K0, int H>
__device__ __forceinline__ void chain(float (&w)[9], const float (&x)[9], float b, int r, float &best, int &bt) {
#pragma unroll
    for (int i = H - 1; i > 0; --i) w[K0 + i] = __fadd_rn(w[K0 + i - 1], x[K0 + i]);
    w[K0] = __fadd_rn(b, x[K0]);
    if (r >= H - 1 && w[K0 + H - 1] > best) {
        best = w[K0 + H - 1];
        bt = r - (H - 1);
    }
}

// The rows scanned for height H: windows t < nt, nt = len + 1 (the pad window) when
// len < T = L - H + 1, else T; so rows r < nt + H - 1 (= len + H or L; never below len).
__device__ __forceinline__ int rows_end(int len, int L, int H) {
    const int T = L - H + 1;
    return len < T ? len + H : L;
}

struct Scan {
    float w[9];          // the two chains: height HA in [0, HA), height 9 - HA behind it
    float pad[9];        // the pad row's sums at the same taps
    float ba, bb, besta, bestb;
    int qa, qb, ta, tb;
};

// rows r0 .. re - 1 of the sentence from the LDS tile (tile row 0 = r0)
template <int HA>
__device__ __forceinline__ void tile_rows(Scan &z, const float *__restrict__ tile, int r0, int re) {
    for (int r = r0; r < re; ++r) {
        const float *x = tile + (r - r0) * kPitch;
        float v[9];
#pragma unroll
        for (int i = 0; i < HA; ++i) v[i] = x[z.qa + i * kCh];
#pragma unroll
        for (int i = 0; i < 9 - HA; ++i) v[HA + i] = x[z.qb + i * kCh];
        chain<0, HA>(z.w, v, z.ba, r, z.besta, z.ta);
        chain<HA, 9 - HA>(z.w, v, z.bb, r, z.bestb, z.tb);
    }
}

// the pad rows behind the sentence
template <int HA>
__device__ __forceinline__ void pad_rows(Scan &z, int len, int L) {
    for (int r = len, e = rows_end(len, L, HA); r < e; ++r) chain<0, HA>(z.w, z.pad, z.ba, r, z.besta, z.ta);
    for (int r = len, e = rows_end(len, L, 9 - HA); r < e; ++r) chain<HA, 9 - HA>(z.w, z.pad, z.bb, r, z.bestb, z.tb);
}

// (kThreads, 4): at most 128 VGPRs, so that the five blocks a CU's LDS holds are resident together
// (cfg2's 1,120 sentences are then one round of blocks on 256 CUs)
__global__ __launch_bounds__(kThreads, 4) void k_vocab_pool(int L, int V, const int64_t *__restrict__ ids,
                                                            const int32_t *__restrict__ rowoff,
                                                            const float *__restrict__ TW, int ldtw, Bias bias,
                                                            float *__restrict__ feat, int32_t *__restrict__ arg) {
    __shared__ float4 tile4[kRows * kRow4];
    __shared__ int32_t tok[kMaxL];
    const int s = blockIdx.x;
    const int len = sent_len(rowoff, s, L);
    for (int r = threadIdx.x; r < len; r += kThreads) {
        const int64_t w = ids[(long)s * L + r];
        tok[r] = w < 0 || w >= V ? 0 : (int32_t)w;
    }
    const float *tile = reinterpret_cast<const float *>(tile4);
    const int p = threadIdx.x >> 6;                     // wave-uniform: heights 2 + p and 7 - p
    const int lane = threadIdx.x & 63;
    const int c = lane < kCh ? lane : kCh - 1;          // lanes 50..63 repeat channel 49 and store nothing
    const int ga = p, gb = 5 - p, ha = 2 + p;

    Scan z;
    z.qa = tap_base(ga) * kCh + c, z.qb = tap_base(gb) * kCh + c;
    z.ba = bias.b[ga][c], z.bb = bias.b[gb][c];
    z.besta = z.bestb = -INFINITY;
    z.ta = z.tb = 0;
    {
        const float *pos0 = TW + (long)V * ldtw;        // token 0 at position 0
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int q = k < ha ? z.qa + k * kCh : z.qb + (k - ha) * kCh;
            z.pad[k] = __fadd_rn(TW[q], pos0[q]);
            z.w[k] = 0.f;
        }
    }

    // this thread's vectors of a tile: columns threadIdx.x and threadIdx.x + kThreads of every row
    const int col0 = threadIdx.x, col1 = threadIdx.x + kThreads;
    float4 ahead[kPer];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int r = r0 + k / 2, col = k & 1 ? col1 : col0;
            if (r < len && col < kRow4) ahead[k] = reinterpret_cast<const float4 *>(TW + (long)tok[r] * ldtw)[col];
        }
    };

    __syncthreads();                                    // tok
    fetch(0);
    for (int r0 = 0; r0 < len; r0 += kRows) {
        // the sums a + p of this tile's rows
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int r = r0 + k / 2, col = k & 1 ? col1 : col0;
            if (r < len && col < kRow4) {
                const float4 pv = reinterpret_cast<const float4 *>(TW + ((long)V + r + 1) * ldtw)[col];
                const float4 a = ahead[k];
                tile4[(k / 2) * kRow4 + col] = make_float4(__fadd_rn(a.x, pv.x), __fadd_rn(a.y, pv.y),
                                                           __fadd_rn(a.z, pv.z), __fadd_rn(a.w, pv.w));
            }
        }
        __syncthreads();
        if (r0 + kRows < len) fetch(r0 + kRows);        // the next tile's token rows, under these sums
        const int re = r0 + kRows < len ? r0 + kRows : len;
        if (p == 0) tile_rows<2>(z, tile, r0, re);
        else if (p == 1) tile_rows<3>(z, tile, r0, re);
        else tile_rows<4>(z, tile, r0, re);
        __syncthreads();                                // the tile is rewritten next
    }
    if (p == 0) pad_rows<2>(z, len, L);
    else if (p == 1) pad_rows<3>(z, len, L);
    else pad_rows<4>(z, len, L);

    if (lane < kCh) {
        const long o = (long)s * kFeat;
        feat[o + ga * kCh + c] = z.besta > 0.f ? z.besta : 0.f;
        arg[o + ga * kCh + c] = z.ta;
        feat[o + gb * kCh + c] = z.bestb > 0.f ? z.bestb : 0.f;
        arg[o + gb * kCh + c] = z.tb;
    }
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int hsg_cnn_vocab_supported(int L) { return L >= 7 && L <= kMaxL ? 1 : 0; }

int hsg_cnn_vocab_pool(int n, int L, int V, const int64_t *ids, const int32_t *rowoff, const float *TW, int ldtw,
                       const float *const *bias, float *feat, int32_t *arg, void *stream) {
    if (n < 0 || L < 7 || L > kMaxL || V < 1 || !rowoff || !bias || ldtw < kNY || ldtw % 4) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!ids || !TW || !feat || !arg || misaligned(TW)) return HSG_EINVAL;
    Bias b;
    for (int g = 0; g < kGroups; ++g) {
        if (!bias[g]) return HSG_EINVAL;
        b.b[g] = bias[g];
    }
    hipLaunchKernelGGL(k_vocab_pool, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, L, V, ids, rowoff, TW,
                       ldtw, b, feat, arg);
    return status();
}

}  // extern "C"
