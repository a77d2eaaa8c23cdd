// hsg_cnn_tokens.hip -- the sentence CNN on distinct tokens and its sparse weight gradient
// for gfx950.  C ABI and the whole contract (values, summation order): include/hsg_cnn_tokens.h.
//
// Forward ("tokens"): X[row] = E[token] + P[position] and the convolution is linear, so the
// GEMM runs over Tb = [the batch's distinct embedding rows ; the L + 1 position rows] and the
// pool adds the two TW rows of every tap.  k_tok_mark flags the tokens, the caller's prefix
// sum numbers them, k_tok_table copies the rows, k_tok_pool is k_cnn_pool on the row pairs.
//
// Backward ("dw" and "tokens"): dWall = dY^T X with a dY of one non-zero window per
// (sentence, height, channel).  k_tok_dw sums g * x(s, arg + i) directly: one block per
// (chunk of 64 sentences, 16 columns of D) stages each sentence's x tile in LDS once; wave p
// owns heights 2 + p and 7 - p (9 taps: the three waves carry equal work), lane c one channel,
// so a thread keeps 9 x 16 partial sums in registers over the whole chunk.  k_tok_dw_reduce
// adds the chunk partials in ascending order.  Multiplies and adds are rounded separately
// (__fmul_rn / __fadd_rn): the order contract is restated exactly in numpy float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_cnn_tokens.h"

// hipcc contracts a * b + c into an FMA by default, through __fmul_rn / __fadd_rn too (they are
// plain operators in the HIP headers); the contracts of this file are written in separately
// rounded operations.  The pragma clears the flag on this file's operations; the back end's
// own fusion is switched off with -ffp-contract=off for this file (build.py FILE_FLAGS).
#pragma clang fp contract(off)

namespace {

constexpr int kGroups = 6;      // kernel heights 2..7
constexpr int kCh = 50;         // channels per height
constexpr int kTaps = 27;       // 2 + 3 + ... + 7
constexpr int kNY = kTaps * kCh;
constexpr int kFeat = kGroups * kCh;
constexpr int kChunk = 64;      // sentences per partial (the order contract's constant)
constexpr int kTile = 16;       // columns of D per block
constexpr int kPitch = 20;      // LDS row pitch in floats: 16 rows on distinct banks per b128 group
constexpr int kMaxL = 400;      // 2 buffers x (L + 1) rows x 80 B <= 64 KiB
constexpr int kDwThreads = 192; // three waves: (2,7), (3,6), (4,5)

__host__ __device__ constexpr int tap_base(int g) { return g * (g + 3) / 2; }   // sum_{j<g} (j+2)

bool supported(int L, int D) { return L >= 7 && L <= kMaxL && D >= 4 && D <= 4096 && D % 4 == 0; }

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

__device__ inline int sent_len(const int32_t *__restrict__ rowoff, int s, int L) {
    int len = rowoff[s + 1] - rowoff[s] - 1;
    len = len < 0 ? 0 : len;
    return len > L ? L : len;
}

__global__ __launch_bounds__(256) void k_tok_mark(long total, int V, const int64_t *__restrict__ ids,
                                                  int32_t *__restrict__ present, int32_t *__restrict__ bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) present[0] = 1;
    if (i >= total) return;
    const int64_t v = ids[i];
    if (v < 0 || v >= V) *bad = 1;
    else present[v] = 1;
}

// One wave per source row: v < V an embedding row (copied when present), V + p position p.
__global__ __launch_bounds__(256) void k_tok_table(int V, int D, int U, int L, const int32_t *__restrict__ present,
                                                   const int32_t *__restrict__ slot, const float *__restrict__ E,
                                                   const float *__restrict__ P, float *__restrict__ Tb, int ldt) {
    const int lane = threadIdx.x & 63;
    const long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= (long)V + L + 1) return;
    const float *src;
    long row;
    if (v < V) {
        if (!present[v]) return;
        row = slot[v];
        if (row < 0 || row >= U) return;
        src = E + v * D;
    } else {
        row = U + (v - V);
        src = P + (v - V) * D;
    }
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
    float4 *d4 = reinterpret_cast<float4 *>(Tb + row * ldt);
    for (int d = lane; d < D / 4; d += 64) d4[d] = s4[d];
}

struct Bias {
    const float *b[kGroups];
};

// One block per sentence, thread (g, c); the sentence's TW row numbers sit in LDS:
// rw[r] = slot of token r for r < len, rw[len] = slot[0].
__global__ __launch_bounds__(320) void k_tok_pool(int L, int V, int U, const int64_t *__restrict__ ids,
                                                  const int32_t *__restrict__ rowoff, const int32_t *__restrict__ slot,
                                                  const float *__restrict__ TW, int ldtw, Bias bias,
                                                  float *__restrict__ feat, int32_t *__restrict__ arg) {
    extern __shared__ int32_t rw[];
    const int s = blockIdx.x;
    const int len = sent_len(rowoff, s, L);
    for (int r = threadIdx.x; r <= len; r += blockDim.x) {
        int64_t w = r < len ? ids[(long)s * L + r] : 0;
        if (w < 0 || w >= V) w = 0;
        int sl = slot[w];
        rw[r] = sl < 0 || sl >= U ? 0 : sl;
    }
    __syncthreads();
    const int gc = threadIdx.x;
    if (gc >= kFeat) return;
    const int g = gc / kCh, c = gc - g * kCh, h = g + 2;
    const int T = L - h + 1;
    const float b = bias.b[g][c];
    const float *col = TW + tap_base(g) * kCh + c;
    const float *pos = col + (long)U * ldtw;
    const int padrow = rw[len];
    float best = -INFINITY;
    int bt = 0;
    const int tv = len < T ? len : T;
    for (int t = 0; t < tv; ++t) {
        float v = b;
        for (int i = 0; i < h; ++i) {
            const int r = t + i;
            const bool real = r < len;
            const float a = col[(long)(real ? rw[r] : padrow) * ldtw + i * kCh];
            const float p = pos[(long)(real ? r + 1 : 0) * ldtw + i * kCh];
            v = __fadd_rn(v, __fadd_rn(a, p));
        }
        if (v > best) { best = v; bt = t; }
    }
    if (len < T) {                                 // the all-padding windows (identical): t = len
        float v = b;
        for (int i = 0; i < h; ++i)
            v = __fadd_rn(v, __fadd_rn(col[(long)padrow * ldtw + i * kCh], pos[i * kCh]));
        if (v > best) { best = v; bt = len; }
    }
    feat[(long)s * kFeat + gc] = best > 0.f ? best : 0.f;
    arg[(long)s * kFeat + gc] = bt;
}

// acc[k][:] += g * x(row arg + k) for the h taps of one height; acc rows k0 .. k0 + h - 1.
template <int K0, int H>
__device__ __forceinline__ void taps(float (&acc)[9][kTile], const float *__restrict__ xs, int len, int t, float g) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const int r = t + i;
        const float4 *x4 = reinterpret_cast<const float4 *>(xs + ((unsigned)r < (unsigned)len ? r : len) * kPitch);
#pragma unroll
        for (int j = 0; j < kTile / 4; ++j) {
            const float4 x = x4[j];
            acc[K0 + i][4 * j + 0] = __fadd_rn(acc[K0 + i][4 * j + 0], __fmul_rn(g, x.x));
            acc[K0 + i][4 * j + 1] = __fadd_rn(acc[K0 + i][4 * j + 1], __fmul_rn(g, x.y));
            acc[K0 + i][4 * j + 2] = __fadd_rn(acc[K0 + i][4 * j + 2], __fmul_rn(g, x.z));
            acc[K0 + i][4 * j + 3] = __fadd_rn(acc[K0 + i][4 * j + 3], __fmul_rn(g, x.w));
        }
    }
}

template <int HA>
__device__ __forceinline__ void pair(float (&acc)[9][kTile], const float *__restrict__ xs, int len, int tA, float gA,
                                     int tB, float gB) {
    if (gA != 0.f) taps<0, HA>(acc, xs, len, tA, gA);
    if (gB != 0.f) taps<HA, 9 - HA>(acc, xs, len, tB, gB);
}

// grid (tiles of D, chunks); ws [chunks][1350][D] then [chunks][300] (the dbias partials,
// written by the tile-0 blocks).
__global__ __launch_bounds__(kDwThreads) void k_tok_dw(int n, int L, int V, int D, const int64_t *__restrict__ ids,
                                                       const int32_t *__restrict__ rowoff,
                                                       const float *__restrict__ E, const float *__restrict__ P,
                                                       const float *__restrict__ feat, const int32_t *__restrict__ arg,
                                                       const float *__restrict__ dfeat, float *__restrict__ ws,
                                                       float *__restrict__ wsb) {
    extern __shared__ float4 xbuf4[];
    float *xbuf = reinterpret_cast<float *>(xbuf4);
    const int d0 = blockIdx.x * kTile;
    const int chunk = blockIdx.y;
    const int s0 = chunk * kChunk;
    const int s1 = s0 + kChunk < n ? s0 + kChunk : n;
    const int p = threadIdx.x >> 6, c = threadIdx.x & 63;
    const bool owner = c < kCh;
    const int colA = p * kCh + c, colB = (5 - p) * kCh + c;     // heights 2 + p and 7 - p

    float acc[9][kTile];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < kTile; ++j) acc[k][j] = 0.f;
    float bA = 0.f, bB = 0.f;

    float nfA = 0.f, nfB = 0.f, ngA = 0.f, ngB = 0.f;
    int ntA = 0, ntB = 0;
    if (owner) {
        const long o = (long)s0 * kFeat;
        nfA = feat[o + colA], nfB = feat[o + colB];
        ngA = dfeat[o + colA], ngB = dfeat[o + colB];
        ntA = arg[o + colA], ntB = arg[o + colB];
    }
    for (int s = s0; s < s1; ++s) {
        float *xs = xbuf + ((s - s0) & 1) * (L + 1) * kPitch;
        const int len = sent_len(rowoff, s, L);
        // stage x(s, r)[d0 .. d0 + 15] for r = 0 .. len (row len = the pad row)
        for (int item = threadIdx.x; item < (len + 1) * (kTile / 4); item += kDwThreads) {
            const int r = item >> 2, col = d0 + 4 * (item & 3);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col < D) {
                const int64_t w = r < len ? ids[(long)s * L + r] : 0;
                const float4 pv = *reinterpret_cast<const float4 *>(P + (long)(r < len ? r + 1 : 0) * D + col);
                if (w < 0 || w >= V) {
                    x = make_float4(NAN, NAN, NAN, NAN);
                } else {
                    const float4 ev = *reinterpret_cast<const float4 *>(E + w * D + col);
                    x = make_float4(__fadd_rn(ev.x, pv.x), __fadd_rn(ev.y, pv.y), __fadd_rn(ev.z, pv.z),
                                    __fadd_rn(ev.w, pv.w));
                }
            }
            *reinterpret_cast<float4 *>(xs + r * kPitch + 4 * (item & 3)) = x;
        }
        const float gA = nfA > 0.f ? ngA : 0.f, gB = nfB > 0.f ? ngB : 0.f;
        const int tA = ntA, tB = ntB;
        if (owner && s + 1 < s1) {                  // the next sentence's operands, under this one's sums
            const long o = (long)(s + 1) * kFeat;
            nfA = feat[o + colA], nfB = feat[o + colB];
            ngA = dfeat[o + colA], ngB = dfeat[o + colB];
            ntA = arg[o + colA], ntB = arg[o + colB];
        }
        // one barrier per sentence: the buffer written two sentences later is this one, and
        // every wave has passed the next barrier (so finished these sums) by then
        __syncthreads();
        if (owner) {
            if (gA != 0.f) bA = __fadd_rn(bA, gA);
            if (gB != 0.f) bB = __fadd_rn(bB, gB);
            if (p == 0) pair<2>(acc, xs, len, tA, gA, tB, gB);
            else if (p == 1) pair<3>(acc, xs, len, tA, gA, tB, gB);
            else pair<4>(acc, xs, len, tA, gA, tB, gB);
        }
    }
    if (!owner) return;
    const int hA = 2 + p;
    float *out = ws + (long)chunk * kNY * D;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int q = k < hA ? (tap_base(p) + k) * kCh + c : (tap_base(5 - p) + k - hA) * kCh + c;
        float4 *o4 = reinterpret_cast<float4 *>(out + (long)q * D + d0);
#pragma unroll
        for (int j = 0; j < kTile / 4; ++j)
            if (d0 + 4 * j < D) o4[j] = make_float4(acc[k][4 * j], acc[k][4 * j + 1], acc[k][4 * j + 2], acc[k][4 * j + 3]);
    }
    if (blockIdx.x == 0) {
        wsb[(long)chunk * kFeat + colA] = bA;
        wsb[(long)chunk * kFeat + colB] = bB;
    }
}

// dWall[q][d .. d+3] and dbias: the chunk partials in ascending order (+0.0 without chunks).
__global__ __launch_bounds__(256) void k_tok_dw_reduce(int chunks, int D, const float *__restrict__ ws,
                                                       const float *__restrict__ wsb, float *__restrict__ dWall,
                                                       int lddw, float *__restrict__ dbias) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int d4 = D / 4;
    const long nw = (long)kNY * d4;
    if (i < nw) {
        const long q = i / d4;
        const int d = (int)(i - q * d4) * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < chunks; ++k) {
            const float4 v = *reinterpret_cast<const float4 *>(ws + ((long)k * kNY + q) * D + d);
            a = k ? make_float4(__fadd_rn(a.x, v.x), __fadd_rn(a.y, v.y), __fadd_rn(a.z, v.z), __fadd_rn(a.w, v.w))
                  : v;
        }
        *reinterpret_cast<float4 *>(dWall + q * lddw + d) = a;
    } else if (i < nw + kFeat) {
        const int j = (int)(i - nw);
        float a = 0.f;
        for (int k = 0; k < chunks; ++k) a = k ? __fadd_rn(a, wsb[(long)k * kFeat + j]) : wsb[j];
        dbias[j] = a;
    }
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int hsg_cnn_tok_supported(int L, int D) { return supported(L, D) ? 1 : 0; }

int hsg_cnn_tok_chunk(void) { return kChunk; }

size_t hsg_cnn_tok_dw_ws_floats(int n, int D) {
    if (n <= 0 || D < 4 || D > 4096 || D % 4) return 0;
    return (size_t)((n + kChunk - 1) / kChunk) * ((size_t)kNY * D + kFeat);
}

int hsg_cnn_tok_mark(int n, int L, int V, const int64_t *ids, int32_t *present, int32_t *bad, void *stream) {
    if (n < 0 || L < 1 || V < 1 || !present || !bad || (n && !ids)) return HSG_EINVAL;
    const long total = (long)n * L;
    const long blocks = total ? (total + 255) / 256 : 1;
    if (blocks > 0x7fffffffL) return HSG_EINVAL;
    hipLaunchKernelGGL(k_tok_mark, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, V, ids, present,
                       bad);
    return status();
}

int hsg_cnn_tok_table(int V, int D, int U, int L, const int32_t *present, const int32_t *slot, const float *E,
                      const float *P, float *Tb, int ldt, void *stream) {
    if (V < 1 || U < 1 || U > V || L < 0 || D < 4 || D > 4096 || D % 4 || ldt < D || ldt % 4) return HSG_EINVAL;
    if (!present || !slot || !E || !P || !Tb || misaligned(E) || misaligned(P) || misaligned(Tb)) return HSG_EINVAL;
    const long rows = (long)V + L + 1;
    hipLaunchKernelGGL(k_tok_table, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, V, D, U, L,
                       present, slot, E, P, Tb, ldt);
    return status();
}

int hsg_cnn_tok_pool(int n, int L, int V, int U, const int64_t *ids, const int32_t *rowoff, const int32_t *slot,
                     const float *TW, int ldtw, const float *const *bias, float *feat, int32_t *arg, void *stream) {
    if (n < 0 || L < 7 || L > kMaxL || V < 1 || U < 1 || U > V || !rowoff || !bias || ldtw < kNY) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!ids || !slot || !TW || !feat || !arg) return HSG_EINVAL;
    Bias b;
    for (int g = 0; g < kGroups; ++g) {
        if (!bias[g]) return HSG_EINVAL;
        b.b[g] = bias[g];
    }
    hipLaunchKernelGGL(k_tok_pool, dim3((unsigned)n), dim3(320), (size_t)(L + 1) * sizeof(int32_t),
                       (hipStream_t)stream, L, V, U, ids, rowoff, slot, TW, ldtw, b, feat, arg);
    return status();
}

int hsg_cnn_tok_dw(int n, int L, int V, int D, const int64_t *ids, const int32_t *rowoff, const float *E,
                   const float *P, const float *feat, const int32_t *arg, const float *dfeat, float *ws,
                   float *dWall, int lddw, float *dbias, void *stream) {
    if (n < 0 || V < 1 || !supported(L, D) || lddw < D || lddw % 4 || !dWall || !dbias || misaligned(dWall))
        return HSG_EINVAL;
    if (n && (!ids || !rowoff || !E || !P || !feat || !arg || !dfeat || !ws || misaligned(E) || misaligned(P) ||
              misaligned(ws)))
        return HSG_EINVAL;
    const int chunks = (n + kChunk - 1) / kChunk;
    if (chunks > 65535) return HSG_EINVAL;
    float *wsb = n ? ws + (size_t)chunks * kNY * D : nullptr;
    if (n) {
        const size_t lds = 2 * (size_t)(L + 1) * kPitch * sizeof(float);
        hipLaunchKernelGGL(k_tok_dw, dim3((unsigned)((D + kTile - 1) / kTile), (unsigned)chunks), dim3(kDwThreads), lds,
                           (hipStream_t)stream, n, L, V, D, ids, rowoff, E, P, feat, arg, dfeat, ws, wsb);
        const int rc = status();
        if (rc) return rc;
    }
    const long total = (long)kNY * (D / 4) + kFeat;
    hipLaunchKernelGGL(k_tok_dw_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chunks,
                       D, ws, wsb, dWall, lddw, dbias);
    return status();
}

}  // extern "C"
