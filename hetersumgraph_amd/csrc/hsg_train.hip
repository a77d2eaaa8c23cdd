// hsg_train.hip -- the training-step tail (train.py:115-119, 132-135) for gfx950: the
// per-document cross entropy, the multi-tensor gradient norm, and clip + Adam.
// C ABI: include/hsg_train.h.
//
// The work is small (a [~1000, 2] cross entropy; ~1.8 M parameters in 55 tensors) and its
// cost in the eager step is launches and host glue, so the design is about launch count:
//
//   hsg_doc_ce     one block per document (its rows' losses and gradients, the document
//                  sum through a fixed tree), then a one-block finish for the mean.
//   hsg_mt_sqnorm  one block per 4,096-element chunk of one tensor -> one fp32 partial.
//   hsg_mt_adam    the same blocks; each sums all partials itself, in double and in one
//                  fixed order, so every block holds the same norm without a hand-off.
//
// The multi-tensor kernels take their table of tensors in the kernel arguments (MtArgs,
// by value): the descriptors and the first block of each.  A block finds its tensor by a
// binary search over those block offsets (wave-uniform: scalar loads of the arguments).
//
// Arithmetic follows torch.optim.Adam's single-tensor path operation by operation with
// floating-point contraction off, so that the fp32 result differs from torch's by the
// rounding of the scalar factors only; sums run in fixed orders and there are no atomics,
// so results are bitwise reproducible and do not depend on the tensors' alignment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_train.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMtK = 64;               // descriptors per launch
constexpr int kChunk = 4096;           // elements per block
constexpr int kGroups = kChunk / (4 * kThreads);   // 4-element groups per thread

struct MtArgs {
    hsg_mt_tensor t[kMtK];
    int32_t first[kMtK + 1];           // first block of tensor i in this launch; first[count] = blocks
    int32_t count;
};
static_assert(sizeof(MtArgs) == 2824, "kernel-argument size documented in hsg_train.h");

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// ---- fixed-order block sums ---------------------------------------------------------
// s[kThreads] holds one value per thread; a binary tree over the thread index.
template <typename T>
__device__ __forceinline__ T block_tree_sum(T *s, T x) {
    const int t = (int)threadIdx.x;
    s[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}

// ---- per-document cross entropy -------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_doc_ce(int n, int B, const float *__restrict__ logits,
                                                     const int64_t *__restrict__ labels, int L, int64_t N,
                                                     const int64_t *__restrict__ rows,
                                                     const int32_t *__restrict__ doc_off,
                                                     float *__restrict__ row_loss, float *__restrict__ doc_loss,
                                                     float *__restrict__ dlogits) {
    __shared__ float s[kThreads];
    const int d = (int)blockIdx.x;
    int beg = doc_off[d], end = doc_off[d + 1];
    beg = beg < 0 ? 0 : (beg > n ? n : beg);
    end = end < beg ? beg : (end > n ? n : end);
    const float invB = 1.f / (float)B;
    float acc = 0.f;
    for (int r = beg + (int)threadIdx.x; r < end; r += kThreads) {
        int64_t lab;
        bool ok = true;
        if (rows) {
            const int64_t node = rows[r];
            lab = 0;
            ok = node >= 0 && node < N;
            if (ok)
                for (int j = 0; j < L; ++j) lab += labels[node * L + j];
        } else {
            lab = labels[r];
        }
        ok = ok && (lab == 0 || lab == 1);
        const float2 z = reinterpret_cast<const float2 *>(logits)[r];
        float loss, g0, g1;
        if (ok) {
            // loss = log(1 + exp(dz)), dz = z_other - z_label; d loss / d z_other = sigmoid(dz)
            const float dz = lab == 1 ? z.x - z.y : z.y - z.x;
            const float e = expf(-fabsf(dz));
            loss = fmaxf(dz, 0.f) + log1pf(e);
            const float q = (dz >= 0.f ? 1.f : e) / (1.f + e);     // sigmoid(dz)
            const float gq = q * invB;
            g0 = lab == 1 ? gq : -gq;
            g1 = -g0;
        } else {
            loss = __builtin_nanf("");
            g0 = g1 = 0.f;
        }
        row_loss[r] = loss;
        reinterpret_cast<float2 *>(dlogits)[r] = make_float2(g0, g1);
        acc += loss;
    }
    const float tot = block_tree_sum(s, acc);
    if (threadIdx.x == 0) doc_loss[d] = tot;
}

__global__ __launch_bounds__(kThreads) void k_doc_mean(int B, const float *__restrict__ doc_loss,
                                                       float *__restrict__ mean) {
    __shared__ float s[kThreads];
    float acc = 0.f;
    for (int d = (int)threadIdx.x; d < B; d += kThreads) acc += doc_loss[d];
    const float tot = block_tree_sum(s, acc);
    if (threadIdx.x == 0) mean[0] = tot / (float)B;
}

// ---- multi-tensor helpers -----------------------------------------------------------
// The tensor that owns block b (wave-uniform) and the chunk's first element in it.
__device__ __forceinline__ int mt_find(const MtArgs &a, int b) {
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// x[0..3] = src[e .. e+3] where e + k < n (0 elsewhere); vec: one 16-byte load.
__device__ __forceinline__ void ld4(float (&x)[4], const float *src, int64_t e, int64_t n, bool vec) {
    if (vec && e + 3 < n) {
        const float4 q = *reinterpret_cast<const float4 *>(src + e);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = e + k < n ? src[e + k] : 0.f;
    }
}

__device__ __forceinline__ void st4(const float (&x)[4], float *dst, int64_t e, int64_t n, bool vec) {
    if (vec && e + 3 < n) {
        *reinterpret_cast<float4 *>(dst + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n) dst[e + k] = x[k];
    }
}

__global__ __launch_bounds__(kThreads) void k_mt_sqnorm(const MtArgs a, float *__restrict__ partials,
                                                        double *__restrict__ step) {
    __shared__ float s[kThreads];
    const int b = (int)blockIdx.x;
    const int i = mt_find(a, b);
    const float *g = a.t[i].g;
    const int64_t n = a.t[i].n;
    const int64_t c0 = (int64_t)(b - a.first[i]) * kChunk;
    const bool vec = al16(g);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const int64_t e = c0 + 4 * (int64_t)(j * kThreads + (int)threadIdx.x);
        if (e >= n) break;
        float x[4];
        ld4(x, g, e, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += x[k] * x[k];
    }
    const float tot = block_tree_sum(s, acc);
    if (threadIdx.x == 0) {
        partials[b] = tot;
        if (step && b == 0) step[0] += 1.0;       // the step's first launch only passes step
    }
}

struct AdamScalars {
    float coef, omb1, beta2, omb2, wd, step_size, bc2_sqrt, eps;
};

__global__ __launch_bounds__(kThreads) void k_mt_adam(const MtArgs a, const float *__restrict__ partials,
                                                      int n_partials, const double *__restrict__ hyper,
                                                      int scale_only, float *__restrict__ norm_out) {
#pragma clang fp contract(off)
    __shared__ double sd[kThreads];
    __shared__ AdamScalars sc_s;
    double acc = 0.0;
    for (int q = (int)threadIdx.x; q < n_partials; q += kThreads) acc += (double)partials[q];
    const double total = block_tree_sum(sd, acc);
    if (threadIdx.x == 0) {
        const double norm = sqrt(total), max_norm = hyper[5];
        double coef = 1.0;
        if (max_norm >= 0.0) {
            coef = max_norm / (norm + 1e-6);
            coef = coef > 1.0 ? 1.0 : coef;        // NaN stays NaN (torch.clamp)
        }
        AdamScalars sc;
        sc.coef = (float)coef;
        if (!scale_only) {
            const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], t = hyper[6];
            sc.omb1 = (float)(1.0 - b1);
            sc.beta2 = (float)b2;
            sc.omb2 = (float)(1.0 - b2);
            sc.wd = (float)hyper[4];
            sc.step_size = (float)(lr / (1.0 - pow(b1, t)));
            sc.bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
            sc.eps = (float)hyper[3];
        }
        sc_s = sc;
        if (norm_out && blockIdx.x == 0) norm_out[0] = (float)norm;
    }
    __syncthreads();
    const AdamScalars sc = sc_s;

    const int b = (int)blockIdx.x;
    const int i = mt_find(a, b);
    float *p = a.t[i].p;
    const float *g = a.t[i].g;
    float *m = a.t[i].m, *v = a.t[i].v;
    const int64_t n = a.t[i].n;
    const int64_t c0 = (int64_t)(b - a.first[i]) * kChunk;
    const bool vec = al16(p) && al16(g) && (scale_only || (al16(m) && al16(v)));
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const int64_t e = c0 + 4 * (int64_t)(j * kThreads + (int)threadIdx.x);
        if (e >= n) break;
        float gx[4], px[4], mx[4], vx[4];
        ld4(gx, g, e, n, vec);
        if (scale_only) {
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = gx[k] * sc.coef;
            st4(px, p, e, n, vec);
            continue;
        }
        ld4(px, p, e, n, vec);
        ld4(mx, m, e, n, vec);
        ld4(vx, v, e, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gk = gx[k] * sc.coef;
            if (sc.wd != 0.f) gk = gk + sc.wd * px[k];
            mx[k] = mx[k] + sc.omb1 * (gk - mx[k]);
            vx[k] = vx[k] * sc.beta2 + (sc.omb2 * gk) * gk;
            const float denom = sqrtf(vx[k]) / sc.bc2_sqrt + sc.eps;
            px[k] = px[k] - sc.step_size * (mx[k] / denom);
        }
        st4(px, p, e, n, vec);
        st4(mx, m, e, n, vec);
        st4(vx, v, e, n, vec);
    }
}

// Blocks of tensor i, or -1 for a descriptor the kernels must not see.
int64_t mt_tensor_blocks(const hsg_mt_tensor &d, bool need_state, bool need_p) {
    if (d.n < 0) return -1;
    if (d.n == 0) return 0;
    if (!d.g || (need_p && !d.p) || (need_state && (!d.m || !d.v))) return -1;
    return (d.n + kChunk - 1) / kChunk;
}

// Walks the table in launches of at most kMtK non-empty tensors; fn(args, blocks, first
// block overall, launch index).  Returns the total block count or -1.
template <typename F>
int64_t mt_for_each_launch(const hsg_mt_tensor *tensors, int T, bool need_state, bool need_p, F fn) {
    if (T < 0 || (T > 0 && !tensors)) return -1;
    int64_t total = 0;
    for (int i = 0; i < T; ++i) {
        const int64_t nb = mt_tensor_blocks(tensors[i], need_state, need_p);
        if (nb < 0) return -1;
        total += nb;
        if (total > 0x7FFFFFFFL) return -1;
    }
    MtArgs a;
    int64_t base = 0;
    int launch = 0, i = 0;
    while (i < T) {
        a.count = 0;
        int32_t blocks = 0;
        for (; i < T && a.count < kMtK; ++i) {
            if (tensors[i].n == 0) continue;
            a.t[a.count] = tensors[i];
            a.first[a.count++] = blocks;
            blocks += (int32_t)mt_tensor_blocks(tensors[i], false, false);
        }
        if (a.count == 0) break;
        for (int k = a.count; k <= kMtK; ++k) a.first[k] = blocks;
        for (int k = a.count; k < kMtK; ++k) a.t[k] = hsg_mt_tensor{nullptr, nullptr, nullptr, nullptr, 0};
        const int rc = fn(a, blocks, base, launch++);
        if (rc) return -(int64_t)rc - 2;
        base += blocks;
    }
    return total;
}

}  // namespace

extern "C" {

int hsg_doc_ce(int n, int C, int B, const float *logits, const int64_t *labels, int L, int64_t N,
               const int64_t *rows, const int32_t *doc_off, float *row_loss, float *doc_loss, float *mean,
               float *dlogits, void *stream) {
    if (C != 2 || n < 0 || B < 1 || !labels || !doc_off || !doc_loss || !mean) return HSG_EINVAL;
    if (n > 0 && (!logits || !row_loss || !dlogits)) return HSG_EINVAL;
    if (rows && (L < 1 || N < 0)) return HSG_EINVAL;
    if (((uintptr_t)logits & 7) || ((uintptr_t)dlogits & 7)) return HSG_EINVAL;      // float2 rows
    hipLaunchKernelGGL(k_doc_ce, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, n, B, logits, labels, L,
                       N, rows, doc_off, row_loss, doc_loss, dlogits);
    hipLaunchKernelGGL(k_doc_mean, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, B, doc_loss, mean);
    return status();
}

int hsg_mt_tensors_per_launch(void) { return kMtK; }

int hsg_mt_chunk(void) { return kChunk; }

size_t hsg_mt_blocks(const struct hsg_mt_tensor *tensors, int T) {
    const int64_t nb = mt_for_each_launch(tensors, T, false, false,
                                          [](const MtArgs &, int32_t, int64_t, int) { return 0; });
    return nb < 0 ? (size_t)-1 : (size_t)nb;
}

int hsg_mt_sqnorm(const struct hsg_mt_tensor *tensors, int T, float *partials, double *hyper, void *stream) {
    const size_t nb = hsg_mt_blocks(tensors, T);
    if (nb == (size_t)-1 || (nb > 0 && !partials)) return HSG_EINVAL;
    const int64_t rc = mt_for_each_launch(
        tensors, T, false, false, [&](const MtArgs &a, int32_t blocks, int64_t base, int launch) {
            hipLaunchKernelGGL(k_mt_sqnorm, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a,
                               partials + base, (hyper && launch == 0) ? hyper + 6 : (double *)nullptr);
            return status();
        });
    return rc >= 0 ? 0 : rc == -1 ? HSG_EINVAL : (int)(-rc - 2);
}

int hsg_mt_adam(const struct hsg_mt_tensor *tensors, int T, const float *partials, const double *hyper,
                int scale_only, float *norm_out, void *stream) {
    if (!hyper) return HSG_EINVAL;
    const bool so = scale_only != 0;
    // validate the whole table (and count its blocks) before the first launch
    const int64_t nb = mt_for_each_launch(tensors, T, !so, true,
                                          [](const MtArgs &, int32_t, int64_t, int) { return 0; });
    if (nb < 0 || (nb > 0 && !partials)) return HSG_EINVAL;
    const int64_t rc = mt_for_each_launch(
        tensors, T, !so, true, [&](const MtArgs &a, int32_t blocks, int64_t, int launch) {
            hipLaunchKernelGGL(k_mt_adam, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a,
                               partials, (int)nb, hyper, so ? 1 : 0, launch == 0 ? norm_out : (float *)nullptr);
            return status();
        });
    return rc >= 0 ? 0 : rc == -1 ? HSG_EINVAL : (int)(-rc - 2);
}

}  // extern "C"
