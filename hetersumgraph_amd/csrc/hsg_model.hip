// hsg_model.hip -- the model glue around the encoders and the WSWGAT stack for gfx950:
// sentence features (HiGraph.py:130-132, 141, 160, 96), the doc-node initial state
// (HiGraph.py:231-244, 202, 207) and the sentence logits (HiGraph.py:108, 219-227).
// C ABI: include/hsg_model.h.
//
// The matrices are small (1,120 x 300 at most) and the cost in the eager step is the
// number of launches, so each family is one launch forward and one (logits: two)
// backward:
//
//   k_sentfeat_fwd  4 rows per 256-thread block (280 blocks for 1,120 rows).  The rows'
//                   x = ngram + P[pos] and L sit in LDS; the weights stream through LDS in
//                   32-wide k tiles (read coalesced, stored transposed); thread t owns
//                   column t of F = [cnn | lstm] for the 4 rows, then thread (r, c) one
//                   element of S = F Wn^T.
//   k_sentfeat_bwd  the same rows: dF = dS Wn, then dngram | dL columns, the weights read
//                   coalesced as they lie (the backward uses them untransposed).
//   k_docinit_*     a wave per supernode row / sentence; the 64-wide matrix-vector
//                   products take their vector through lane reads, no LDS.
//   k_logits_*      16 lanes per row forward (two outputs per row, summed in double and
//                   rounded once); a wave per supernode row backward, with the weight
//                   partials of 64-row blocks in the same launch.
//
// Every product is summed in fp32 as fmaf chains over 32 consecutive k, the chains' sums
// added in ascending k (a plain chain over K = 300 errs about 5 x the fp32 CPU GEMM's error
// against fp64, the blocked one under 2 x); every sum over rows is a loop in ascending index
// or a fixed tree; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 4;                 // rows per block of the sentence-feature kernels
constexpr int kFn = 128;                 // n_feature_size
constexpr int kHs = 64;                  // hidden_size of the sentence-feature / doc kernels
constexpr int kTK = 32;                  // k tile of the staged weights
constexpr int kWPitch = 2 * kFn + 1;     // LDS pitch of a staged tile row
constexpr int kMaxK = 512;
constexpr int kPartRows = 64;            // rows per weight-partial block of the logits backward

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

// ---- sentence features, forward --------------------------------------------------------
// A weight tile: k [k0, k0 + 32) of kV * 32 weight rows (row i < split from A, width KA, else
// from B, width KB), read coalesced (8 lanes per row, 16 bytes each) into registers by
// tile_load and written transposed, ws[kk][row], by tile_store -- two steps, so the next
// tile's loads are in flight while the current one is consumed.
template <int kV>
__device__ __forceinline__ void tile_load(float4 (&v)[kV], const float *__restrict__ A, int KA,
                                          const float *__restrict__ B, int KB, int split, int k0) {
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int q = i * kThreads + (int)threadIdx.x;
        const int row = q >> 3, k = k0 + 4 * (q & 7);
        const bool a = row < split;
        const int K = a ? KA : KB;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < K) v[i] = *reinterpret_cast<const float4 *>((a ? A + (size_t)row * KA : B + (size_t)(row - split) * KB) + k);
    }
}

template <int kV>
__device__ __forceinline__ void tile_store(float *ws, const float4 (&v)[kV]) {
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int q = i * kThreads + (int)threadIdx.x;
        float *d = ws + (4 * (q & 7)) * kWPitch + (q >> 3);
        d[0] = v[i].x;
        d[kWPitch] = v[i].y;
        d[2 * kWPitch] = v[i].z;
        d[3 * kWPitch] = v[i].w;
    }
}

__global__ __launch_bounds__(kThreads) void k_sentfeat_fwd(
    int n, int E, int Lw, int n_pos, const float *__restrict__ ngram, int ldn, const int64_t *__restrict__ pos,
    const float *__restrict__ P, const float *__restrict__ L, int ldl, const float *__restrict__ Wc,
    const float *__restrict__ bc, const float *__restrict__ Wl, const float *__restrict__ bl,
    const float *__restrict__ Wn, float *__restrict__ X, int ldx, float *__restrict__ F, int ldf,
    float *__restrict__ S, int lds) {
    extern __shared__ float smem[];
    float *xs = smem;                        // [kRows][E]
    float *ls = xs + kRows * E;              // [kRows][Lw]
    float *ws = ls + kRows * Lw;             // [kTK][kWPitch]
    float *fs = ws + kTK * kWPitch;          // [kRows][2*kFn]
    const int t = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * kRows;
    constexpr int kVF = 2 * kFn * (kTK / 4) / kThreads, kVS = kHs * (kTK / 4) / kThreads;
    float4 pf[kVF];
    tile_load<kVF>(pf, Wc, E, Wl, Lw, kFn, 0);

    for (int idx = t; idx < kRows * E; idx += kThreads) {
        const int r = idx / E, k = idx - r * E, row = row0 + r;
        float v = 0.f;
        if (row < n) {
            const int64_t p = pos[row];
            v = (p >= 0 && p < (int64_t)n_pos) ? ngram[(size_t)row * ldn + k] + P[(size_t)p * E + k] : qnan();
            if (X) X[(size_t)row * ldx + k] = v;
        }
        xs[idx] = v;
    }
    for (int idx = t; idx < kRows * Lw; idx += kThreads) {
        const int r = idx / Lw, k = idx - r * Lw, row = row0 + r;
        ls[idx] = row < n ? L[(size_t)row * ldl + k] : 0.f;
    }

    // F: thread t owns column t (cnn_proj for t < Fn, lstm_proj after)
    const bool cnn = t < kFn;
    const int K = cnn ? E : Lw;
    const float *in = cnn ? xs : ls;
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
    const int Kmax = E > Lw ? E : Lw;
    for (int k0 = 0; k0 < Kmax; k0 += kTK) {
        __syncthreads();                     // the rows are staged / the last tile is consumed
        tile_store<kVF>(ws, pf);
        __syncthreads();
        if (k0 + kTK < Kmax) tile_load<kVF>(pf, Wc, E, Wl, Lw, kFn, k0 + kTK);
        const int kend = K - k0 < kTK ? K - k0 : kTK;      // wave-uniform (<= 0: nothing left)
        if (kend <= 0) continue;
        float loc[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) loc[r] = 0.f;
        for (int kk = 0; kk < kend; ++kk) {
            const float w = ws[kk * kWPitch + t];
#pragma unroll
            for (int r = 0; r < kRows; ++r) loc[r] = fmaf(in[r * K + k0 + kk], w, loc[r]);
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] += loc[r];
    }
    float4 ps[kVS];
    tile_load<kVS>(ps, Wn, 2 * kFn, Wn, 2 * kFn, kHs, 0);
    const float b = cnn ? bc[t] : bl[t - kFn];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const float f = acc[r] + b;
        fs[r * 2 * kFn + t] = f;
        if (row0 + r < n) F[(size_t)(row0 + r) * ldf + t] = f;
    }

    // S: thread (r, c) = (t / Hs, t % Hs)
    const int r = t >> 6, c = t & 63;
    float s = 0.f;
    for (int k0 = 0; k0 < 2 * kFn; k0 += kTK) {
        __syncthreads();
        tile_store<kVS>(ws, ps);
        __syncthreads();
        if (k0 + kTK < 2 * kFn) tile_load<kVS>(ps, Wn, 2 * kFn, Wn, 2 * kFn, kHs, k0 + kTK);
        float loc = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < kTK; ++kk) loc = fmaf(fs[r * 2 * kFn + k0 + kk], ws[kk * kWPitch + c], loc);
        s += loc;
    }
    if (row0 + r < n) S[(size_t)(row0 + r) * lds + c] = s;
}

// ---- sentence features, backward -------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sentfeat_bwd(
    int n, int E, int Lw, const float *__restrict__ dS, int ldds, const float *__restrict__ Wc,
    const float *__restrict__ Wl, const float *__restrict__ Wn, float *__restrict__ dF, int lddf,
    float *__restrict__ dngram, int lddn, float *__restrict__ dL, int lddl) {
    __shared__ float ds[kRows * kHs];
    __shared__ float dfs[kRows * 2 * kFn];
    const int t = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * kRows;
    {
        const int r = t >> 6, c = t & 63;
        ds[t] = row0 + r < n ? dS[(size_t)(row0 + r) * ldds + c] : 0.f;
    }
    __syncthreads();
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
    for (int c0 = 0; c0 < kHs; c0 += kTK) {
        float loc[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) loc[r] = 0.f;
        for (int c = c0; c < c0 + kTK; ++c) {
            const float w = Wn[c * 2 * kFn + t];
#pragma unroll
            for (int r = 0; r < kRows; ++r) loc[r] = fmaf(ds[r * kHs + c], w, loc[r]);
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] += loc[r];
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        dfs[r * 2 * kFn + t] = acc[r];
        if (row0 + r < n) dF[(size_t)(row0 + r) * lddf + t] = acc[r];
    }
    __syncthreads();
    for (int o = t; o < E + Lw; o += kThreads) {
        const bool cnn = o < E;
        float *out = cnn ? dngram : dL;
        if (!out) continue;
        const int K = cnn ? E : Lw, col = cnn ? o : o - E, ld = cnn ? lddn : lddl;
        const float *W = (cnn ? Wc : Wl) + col;
        const float *g = dfs + (cnn ? 0 : kFn);
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
        for (int j0 = 0; j0 < kFn; j0 += kTK) {
            float loc[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) loc[r] = 0.f;
            for (int j = j0; j < j0 + kTK; ++j) {
                const float w = W[(size_t)j * K];
#pragma unroll
                for (int r = 0; r < kRows; ++r) loc[r] = fmaf(g[r * 2 * kFn + j], w, loc[r]);
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] += loc[r];
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (row0 + r < n) out[(size_t)(row0 + r) * ld + col] = acc[r];
    }
}

// ---- doc-node initial state -------------------------------------------------------------
// y[c] = sum_k v[k] * W[c][k] (transposed = false) or sum_k v[k] * W[k][c] (true); v is held
// one element per lane, W is [64][64].  Wave-uniform control flow only.
template <bool kTrans>
__device__ __forceinline__ float wave_matvec64(float v, const float *__restrict__ W, int c) {
    float y = 0.f;
    for (int k0 = 0; k0 < kHs; k0 += kTK) {
        float loc = 0.f;
#pragma unroll 8
        for (int k = k0; k < k0 + kTK; ++k) loc = fmaf(__shfl(v, k, 64), kTrans ? W[k * kHs + c] : W[c * kHs + k], loc);
        y += loc;
    }
    return y;
}

__global__ __launch_bounds__(kThreads) void k_docinit_fwd(
    int n_s, int n_docs, int n_super, const float *__restrict__ S, int lds, const int32_t *__restrict__ super_src,
    const int32_t *__restrict__ doc_ptr, const int32_t *__restrict__ doc_sent, const float *__restrict__ inv_cnt,
    const float *__restrict__ Wd, float *__restrict__ mean, float *__restrict__ init, int ldi) {
    const int c = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * (kThreads / 64) + ((int)threadIdx.x >> 6);      // wave-uniform
    if (row >= n_super) return;
    const int v = super_src[row];
    float out;
    if (v >= 0) {
        out = v < n_s ? S[(size_t)v * lds + c] : qnan();
    } else {
        const int64_t d = -((int64_t)v + 1);
        if (d >= n_docs) {
            out = qnan();
        } else {
            float a = 0.f;
            const int beg = doc_ptr[d], end = doc_ptr[d + 1];
            for (int e = beg; e < end; ++e) {
                const int s = doc_sent[e];
                a += (s >= 0 && s < n_s) ? S[(size_t)s * lds + c] : qnan();
            }
            const float m = a * inv_cnt[d];
            mean[(size_t)d * kHs + c] = m;
            out = wave_matvec64<false>(m, Wd, c);
        }
    }
    init[(size_t)row * ldi + c] = out;
}

__global__ __launch_bounds__(kThreads) void k_docinit_bwd(
    int n_s, int n_docs, int n_super, int sent_blocks, const float *__restrict__ dInit, int ldd,
    const int32_t *__restrict__ sent_row, const int32_t *__restrict__ doc_row,
    const int32_t *__restrict__ sent_ptr, const int32_t *__restrict__ sent_doc,
    const float *__restrict__ inv_cnt, const float *__restrict__ Wd, const float *__restrict__ mean,
    float *__restrict__ dS, int ldds, float *__restrict__ dWd) {
    if ((int)blockIdx.x >= sent_blocks) {
        // dWd[i][j] = sum_d dInit[doc_row[d]][i] * mean[d][j], docs ascending
        const int idx = ((int)blockIdx.x - sent_blocks) * kThreads + (int)threadIdx.x;
        const int i = idx >> 6, j = idx & 63;
        float a = 0.f;
        for (int d = 0; d < n_docs; ++d) {
            const int rd = doc_row[d];
            const float g = (rd >= 0 && rd < n_super) ? dInit[(size_t)rd * ldd + i] : qnan();
            a = fmaf(g, mean[(size_t)d * kHs + j], a);
        }
        dWd[idx] = a;
        return;
    }
    const int c = (int)threadIdx.x & 63;
    const int s = (int)blockIdx.x * (kThreads / 64) + ((int)threadIdx.x >> 6);        // wave-uniform
    if (s >= n_s) return;
    const int rs = sent_row[s];
    float a = (rs >= 0 && rs < n_super) ? dInit[(size_t)rs * ldd + c] : 0.f;
    const int beg = sent_ptr[s], end = sent_ptr[s + 1];
    for (int e = beg; e < end; ++e) {
        const int d = sent_doc[e];
        const int rd = (d >= 0 && d < n_docs) ? doc_row[d] : -1;
        if (rd < 0 || rd >= n_super) {
            a = qnan();
            continue;
        }
        const float g = wave_matvec64<true>(dInit[(size_t)rd * ldd + c], Wd, c);
        a = fmaf(inv_cnt[d], g, a);
    }
    dS[(size_t)s * ldds + c] = a;
}

// ---- sentence logits --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_logits_fwd(
    int n, int Hs, int W, int n_super, const float *__restrict__ state, int ldst,
    const int32_t *__restrict__ sent_super, const int32_t *__restrict__ doc_super, const float *__restrict__ Wh,
    const float *__restrict__ bh, float *__restrict__ logits) {
    const int l16 = (int)threadIdx.x & 15;
    const int row = (int)blockIdx.x * (kThreads / 16) + ((int)threadIdx.x >> 4);
    const bool live = row < n;
    // two outputs per row: the sums are kept in double (a product of two floats is exact
    // there) and rounded to fp32 once, after the bias
    double p0 = 0.0, p1 = 0.0;
    bool bad = false;
    if (live) {
        const int a = sent_super ? sent_super[row] : row;
        if (a < 0 || a >= n_super) {
            bad = true;
        } else {
            const float *x = state + (size_t)a * ldst;
            for (int c = l16 * 4; c < Hs; c += 64)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p0 = fma((double)x[c + j], (double)Wh[c + j], p0);
                    p1 = fma((double)x[c + j], (double)Wh[W + c + j], p1);
                }
        }
        if (doc_super) {
            const int b = doc_super[row];
            if (b < 0 || b >= n_super) {
                bad = true;
            } else {
                const float *x = state + (size_t)b * ldst;
                for (int c = l16 * 4; c < Hs; c += 64)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        p0 = fma((double)x[c + j], (double)Wh[Hs + c + j], p0);
                        p1 = fma((double)x[c + j], (double)Wh[W + Hs + c + j], p1);
                    }
            }
        }
    }
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) {
        p0 += __shfl_xor(p0, m, 16);
        p1 += __shfl_xor(p1, m, 16);
    }
    if (live && l16 == 0) {
        logits[2 * (size_t)row] = bad ? qnan() : (float)(p0 + (double)bh[0]);
        logits[2 * (size_t)row + 1] = bad ? qnan() : (float)(p1 + (double)bh[1]);
    }
}

__global__ __launch_bounds__(kThreads) void k_logits_bwd(
    int n, int Hs, int W, int n_super, int row_blocks, const float *__restrict__ dlogits,
    const float *__restrict__ state, int ldst, const int32_t *__restrict__ sent_super,
    const int32_t *__restrict__ doc_super, const int32_t *__restrict__ sup_sent,
    const int32_t *__restrict__ sup_ptr, const int32_t *__restrict__ sup_list, const float *__restrict__ Wh,
    float *__restrict__ dstate, int ldd, float *__restrict__ ws) {
    if ((int)blockIdx.x >= row_blocks) {
        // weight partials of rows [i0, i1): ws[b][k*W + c] = sum_i dlogits[i][k] * in_i[c],
        // ws[b][2W + k] = sum_i dlogits[i][k]
        const int b = (int)blockIdx.x - row_blocks;
        const int i0 = b * kPartRows, i1 = i0 + kPartRows < n ? i0 + kPartRows : n;
        for (int o = (int)threadIdx.x; o < 2 * W + 2; o += kThreads) {
            float a = 0.f;
            if (o >= 2 * W) {
                for (int i = i0; i < i1; ++i) a += dlogits[2 * (size_t)i + (o - 2 * W)];
            } else {
                const int k = o / W, c = o - k * W;
                const bool second = c >= Hs;
                for (int i = i0; i < i1; ++i) {
                    const int src = second ? doc_super[i] : (sent_super ? sent_super[i] : i);
                    const float x = (src >= 0 && src < n_super) ? state[(size_t)src * ldst + (second ? c - Hs : c)]
                                                                : qnan();
                    a = fmaf(dlogits[2 * (size_t)i + k], x, a);
                }
            }
            ws[(size_t)b * (2 * W + 2) + o] = a;
        }
        return;
    }
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * (kThreads / 64) + ((int)threadIdx.x >> 6);        // wave-uniform
    if (r >= n_super) return;
    for (int c = lane; c < Hs; c += 64) {
        float a = 0.f;
        if (!sent_super) {
            a = fmaf(dlogits[2 * (size_t)r + 1], Wh[W + c], dlogits[2 * (size_t)r] * Wh[c]);
        } else {
            const int i = sup_sent[r];
            if (i >= 0 && i < n) a = fmaf(dlogits[2 * (size_t)i + 1], Wh[W + c], dlogits[2 * (size_t)i] * Wh[c]);
            const int beg = sup_ptr[r], end = sup_ptr[r + 1];
            for (int e = beg; e < end; ++e) {
                const int j = sup_list[e];
                if (j < 0 || j >= n) {
                    a = qnan();
                    continue;
                }
                a += fmaf(dlogits[2 * (size_t)j + 1], Wh[W + Hs + c], dlogits[2 * (size_t)j] * Wh[Hs + c]);
            }
        }
        dstate[(size_t)r * ldd + c] = a;
    }
}

__global__ __launch_bounds__(kThreads) void k_logits_bwd_finish(int blocks, int W, const float *__restrict__ ws,
                                                                float *__restrict__ dWh, float *__restrict__ dbh) {
    const int o = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (o >= 2 * W + 2) return;
    float a = 0.f;
    for (int b = 0; b < blocks; ++b) a += ws[(size_t)b * (2 * W + 2) + o];
    if (o < 2 * W) dWh[o] = a; else dbh[o - 2 * W] = a;
}

size_t sentfeat_lds(int E, int Lw) { return sizeof(float) * (size_t)(kRows * (E + Lw) + kTK * kWPitch + kRows * 2 * kFn); }

}  // namespace

extern "C" {

int hsg_sentfeat_supported(int E, int Fn, int Lw, int Hs) {
    return Fn == kFn && Hs == kHs && E >= 4 && E <= kMaxK && E % 4 == 0 && Lw >= 4 && Lw <= kMaxK && Lw % 4 == 0;
}

int hsg_sentfeat_rows(void) { return kRows; }

int hsg_sentfeat_fwd(int n, int E, int Fn, int Lw, int Hs, int n_pos, const float *ngram, int ldn,
                     const int64_t *pos, const float *P, const float *L, int ldl, const float *Wc, const float *bc,
                     const float *Wl, const float *bl, const float *Wn, float *X, int ldx, float *F, int ldf,
                     float *S, int lds, void *stream) {
    if (n < 0 || n_pos < 0 || !hsg_sentfeat_supported(E, Fn, Lw, Hs)) return HSG_EINVAL;
    if (ldn < E || ldl < Lw || ldf < 2 * Fn || lds < Hs || (X && ldx < E)) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!ngram || !pos || !P || !L || !Wc || !bc || !Wl || !bl || !Wn || !F || !S) return HSG_EINVAL;
    if (!al16(Wc) || !al16(Wl) || !al16(Wn)) return HSG_EINVAL;
    hipLaunchKernelGGL(k_sentfeat_fwd, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), sentfeat_lds(E, Lw),
                       (hipStream_t)stream, n, E, Lw, n_pos, ngram, ldn, pos, P, L, ldl, Wc, bc, Wl, bl, Wn, X, ldx,
                       F, ldf, S, lds);
    return status();
}

int hsg_sentfeat_bwd(int n, int E, int Fn, int Lw, int Hs, const float *dS, int ldds, const float *Wc,
                     const float *Wl, const float *Wn, float *dF, int lddf, float *dngram, int lddn, float *dL,
                     int lddl, void *stream) {
    if (n < 0 || !hsg_sentfeat_supported(E, Fn, Lw, Hs)) return HSG_EINVAL;
    if (ldds < Hs || lddf < 2 * Fn || (dngram && lddn < E) || (dL && lddl < Lw)) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!dS || !Wc || !Wl || !Wn || !dF) return HSG_EINVAL;
    hipLaunchKernelGGL(k_sentfeat_bwd, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), 0,
                       (hipStream_t)stream, n, E, Lw, dS, ldds, Wc, Wl, Wn, dF, lddf, dngram, lddn, dL, lddl);
    return status();
}

int hsg_docinit_supported(int Hs) { return Hs == kHs; }

int hsg_docinit_fwd(int n_s, int n_docs, int n_super, int Hs, const float *S, int lds, const int32_t *super_src,
                    const int32_t *doc_ptr, const int32_t *doc_sent, const float *inv_cnt, const float *Wd,
                    float *mean, float *init, int ldi, void *stream) {
    if (n_s < 0 || n_docs < 0 || n_super < 0 || !hsg_docinit_supported(Hs)) return HSG_EINVAL;
    if (lds < Hs || ldi < Hs) return HSG_EINVAL;
    if (n_super == 0) return 0;
    if (!super_src || !init || (n_s > 0 && !S)) return HSG_EINVAL;
    if (n_docs > 0 && (!doc_ptr || !doc_sent || !inv_cnt || !Wd || !mean)) return HSG_EINVAL;
    const int rows = kThreads / 64;
    hipLaunchKernelGGL(k_docinit_fwd, dim3((unsigned)((n_super + rows - 1) / rows)), dim3(kThreads), 0,
                       (hipStream_t)stream, n_s, n_docs, n_super, S, lds, super_src, doc_ptr, doc_sent, inv_cnt, Wd,
                       mean, init, ldi);
    return status();
}

int hsg_docinit_bwd(int n_s, int n_docs, int n_super, int Hs, const float *dInit, int ldd,
                    const int32_t *sent_row, const int32_t *doc_row, const int32_t *sent_ptr,
                    const int32_t *sent_doc, const float *inv_cnt, const float *Wd, const float *mean, float *dS,
                    int ldds, float *dWd, void *stream) {
    if (n_s < 0 || n_docs < 0 || n_super < 0 || !hsg_docinit_supported(Hs)) return HSG_EINVAL;
    if (ldd < Hs || (dS && ldds < Hs)) return HSG_EINVAL;
    const int rows = kThreads / 64;
    const int sent_blocks = dS ? (n_s + rows - 1) / rows : 0;
    const int w_blocks = dWd ? kHs * kHs / kThreads : 0;
    if (sent_blocks + w_blocks == 0) return 0;
    if (!dInit && n_super > 0) return HSG_EINVAL;
    if (sent_blocks && (!sent_row || !sent_ptr)) return HSG_EINVAL;
    if (n_docs > 0 && (!doc_row || !inv_cnt || !Wd || !mean || (sent_blocks && !sent_doc))) return HSG_EINVAL;
    hipLaunchKernelGGL(k_docinit_bwd, dim3((unsigned)(sent_blocks + w_blocks)), dim3(kThreads), 0,
                       (hipStream_t)stream, n_s, n_docs, n_super, sent_blocks, dInit, ldd, sent_row, doc_row,
                       sent_ptr, sent_doc, inv_cnt, Wd, mean, dS, ldds, dWd);
    return status();
}

int hsg_logits_supported(int Hs) { return Hs >= 4 && Hs <= 256 && Hs % 4 == 0; }

int hsg_logits_fwd(int n, int Hs, int n_super, const float *state, int ldst, const int32_t *sent_super,
                   const int32_t *doc_super, const float *Wh, const float *bh, float *logits, void *stream) {
    if (n < 0 || n_super < 0 || !hsg_logits_supported(Hs) || ldst < Hs) return HSG_EINVAL;
    if ((sent_super == nullptr) != (doc_super == nullptr)) return HSG_EINVAL;
    if (!sent_super && n_super != n) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!state || !Wh || !bh || !logits) return HSG_EINVAL;
    const int rows = kThreads / 16;
    hipLaunchKernelGGL(k_logits_fwd, dim3((unsigned)((n + rows - 1) / rows)), dim3(kThreads), 0, (hipStream_t)stream,
                       n, Hs, sent_super ? 2 * Hs : Hs, n_super, state, ldst, sent_super, doc_super, Wh, bh, logits);
    return status();
}

int hsg_logits_bwd_blocks(int n) { return n <= 0 ? 0 : (n + kPartRows - 1) / kPartRows; }

int hsg_logits_bwd(int n, int Hs, int n_super, const float *dlogits, const float *state, int ldst,
                   const int32_t *sent_super, const int32_t *doc_super, const int32_t *sup_sent,
                   const int32_t *sup_ptr, const int32_t *sup_list, const float *Wh, float *dstate, int ldd,
                   float *ws, float *dWh, float *dbh, void *stream) {
    if (n < 0 || n_super < 0 || !hsg_logits_supported(Hs) || ldst < Hs || (dstate && ldd < Hs)) return HSG_EINVAL;
    if ((sent_super == nullptr) != (doc_super == nullptr)) return HSG_EINVAL;
    if (!sent_super && n_super != n) return HSG_EINVAL;
    const bool want_w = dWh || dbh || ws;
    if (want_w && (!dWh || !dbh || !ws)) return HSG_EINVAL;
    if (n == 0) return 0;
    if (!dlogits || !Wh || (want_w && !state)) return HSG_EINVAL;
    if (sent_super && dstate && (!sup_sent || !sup_ptr || !sup_list)) return HSG_EINVAL;
    const int W = sent_super ? 2 * Hs : Hs;
    const int rows = kThreads / 64;
    const int row_blocks = dstate ? (n_super + rows - 1) / rows : 0;
    const int part_blocks = want_w ? hsg_logits_bwd_blocks(n) : 0;
    if (row_blocks + part_blocks == 0) return 0;
    hipLaunchKernelGGL(k_logits_bwd, dim3((unsigned)(row_blocks + part_blocks)), dim3(kThreads), 0,
                       (hipStream_t)stream, n, Hs, W, n_super, row_blocks, dlogits, state, ldst, sent_super, doc_super,
                       sup_sent, sup_ptr, sup_list, Wh, dstate, ldd, ws);
    if (want_w)
        hipLaunchKernelGGL(k_logits_bwd_finish, dim3((unsigned)((2 * W + 2 + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, (hipStream_t)stream, part_blocks, W, ws, dWh, dbh);
    return status();
}

}  // extern "C"
