// hsg_eval.hip -- the evaluation step's sentence selection (Tester.py:105-140, 155-184) for
// gfx950: per document the candidate order, top-m with or without n-gram blocking, the
// m == 0 argmax rule and the four match counters, in one launch per batch.
// C ABI and the whole contract: include/hsg_eval.h.
//
// The work is tiny (32 to 256 documents of at most 50 rows in every BASELINE config); what
// the eager path pays for is host round trips, so the design is one launch and no read-back:
//
//   k_eval_select  one block of ONE wave per document.  The scores become order-preserving
//                  integer keys in LDS; rank_i = #{j : key_j precedes key_i} by counting; the
//                  blocking walk is serial over the ranked candidates, the lanes striding over
//                  a candidate's ids, the verdict from a 64-bit ballot, the seen set a bitmap
//                  in LDS set with integer atomics.
//
// Dynamic LDS: key[n_max] | order[n_max] | flag[n_max] | bitmap[ceil(gram_max / 32)], at most
// 12 KB + 32 KB.  A block is a single wave, so __syncthreads() orders its LDS traffic at the
// cost of a wait; all control flow around the barriers and ballots is wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_eval.h"

namespace {

constexpr int kWave = 64;
constexpr int kNMax = 1024;
constexpr int kGramMax = 262144;

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// Order-preserving key of a score: a > b as floats <=> key(a) > key(b), -0.0 and 0.0 share a
// key, every NaN shares the largest one.
__device__ __forceinline__ uint32_t score_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    if (x == 0.f) return 0x80000000u;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return __shfl(v, 0, kWave);
}

__global__ __launch_bounds__(kWave) void k_eval_select(int n, const float *__restrict__ logits,
                                                       const int64_t *__restrict__ labels,
                                                       const int32_t *__restrict__ doc_off, int m, int n_max,
                                                       const int32_t *__restrict__ gram_ptr,
                                                       const int32_t *__restrict__ gram_ids,
                                                       const int32_t *__restrict__ gram_cnt, int gram_max,
                                                       int32_t *__restrict__ sel, int sel_ld,
                                                       int32_t *__restrict__ nsel, int32_t *__restrict__ doc_counts,
                                                       unsigned long long *__restrict__ totals) {
    extern __shared__ uint32_t lds[];
    uint32_t *key = lds;                                   // [n_max]
    int32_t *order = reinterpret_cast<int32_t *>(lds + n_max);      // [n_max] rank -> local index
    uint32_t *flag = lds + 2 * n_max;                      // [n_max] 1: selected
    uint32_t *seen = lds + 3 * n_max;                      // [ceil(gram_max / 32)]

    const int d = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int beg = clampi(doc_off[d], 0, n);
    const int end = clampi(doc_off[d + 1], beg, n);
    const int N = end - beg;
    int32_t *srow = sel + (size_t)d * sel_ld;
    const bool blocking = m > 0 && gram_ptr != nullptr;

    // ---- refusals (wave-uniform) ----------------------------------------------------------
    bool ok = N <= n_max;
    int cnt = 0, T = 0;
    if (ok && blocking) {
        cnt = gram_cnt[d];
        ok = cnt >= 0 && cnt <= gram_max;
        T = gram_ptr[n] < 0 ? 0 : gram_ptr[n];
        if (ok) {
            const int lo = clampi(gram_ptr[beg], 0, T);
            const int hi = clampi(gram_ptr[end], lo, T);
            bool bad = false;
            for (int t = lo + lane; t < hi; t += kWave) bad |= (uint32_t)gram_ids[t] >= (uint32_t)cnt;
            ok = !__any(bad);
        }
    }
    if (!ok) {
        for (int c = lane; c < sel_ld; c += kWave) srow[c] = -1;
        if (lane == 0) nsel[d] = -1;
        if (lane < 4) doc_counts[4 * d + lane] = 0;
        return;
    }

    int chosen = 0;
    if (m == 0) {
        // ---- argmax(logits[i]) != 0 with torch's NaN rule, ascending index --------------------
        for (int base = 0; base < N; base += kWave) {
            const int i = base + lane;
            bool p = false;
            if (i < N) {
                const float p0 = logits[2 * (size_t)(beg + i)], p1 = logits[2 * (size_t)(beg + i) + 1];
                p = !(p0 != p0) && ((p1 != p1) || p1 > p0);
                flag[i] = p ? 1u : 0u;
            }
            const unsigned long long mask = __ballot(p);
            if (p) srow[chosen + __popcll(mask & ((1ull << lane) - 1ull))] = i;
            chosen += __popcll(mask);
        }
    } else {
        const int k = m < N ? m : N;
        for (int i = lane; i < N; i += kWave) {
            key[i] = score_key(logits[2 * (size_t)(beg + i) + 1]);
            flag[i] = 0u;
        }
        if (blocking)
            for (int w = lane; w < (cnt + 31) / 32; w += kWave) seen[w] = 0u;
        __syncthreads();
        // ---- ranks by counting: j precedes i iff key_j > key_i, or equal and j < i ------------
        for (int i = lane; i < N; i += kWave) {
            const uint32_t ki = key[i];
            int r = 0;
            for (int j = 0; j < N; ++j) {
                const uint32_t kj = key[j];
                r += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            order[r] = i;                                  // a total order: r is a permutation of 0..N-1
        }
        __syncthreads();
        if (!blocking) {
            for (int c = lane; c < k; c += kWave) {
                const int i = order[c];
                srow[c] = i;
                flag[i] = 1u;
            }
            chosen = k;
        } else {
            // ---- the serial walk of Tester.py:155-184 ------------------------------------------
            for (int c = 0; c < N && chosen < k; ++c) {
                const int i = order[c];
                const int lo = clampi(gram_ptr[beg + i], 0, T);
                const int hi = clampi(gram_ptr[beg + i + 1], lo, T);
                bool hit = false;
                for (int t = lo + lane; t < hi; t += kWave) {
                    const uint32_t id = (uint32_t)gram_ids[t];
                    if (id < (uint32_t)cnt) hit |= (seen[id >> 5] >> (id & 31u)) & 1u;
                }
                if (__any(hit)) continue;                  // wave-uniform
                __syncthreads();                           // every lane tested before any bit is set
                for (int t = lo + lane; t < hi; t += kWave) {
                    const uint32_t id = (uint32_t)gram_ids[t];
                    if (id < (uint32_t)cnt) atomicOr(&seen[id >> 5], 1u << (id & 31u));
                }
                if (lane == 0) {
                    srow[chosen] = i;
                    flag[i] = 1u;
                }
                ++chosen;
                __syncthreads();                           // the bits are visible to the next candidate
            }
        }
    }
    for (int c = chosen + lane; c < sel_ld; c += kWave) srow[c] = -1;
    __syncthreads();

    // ---- counters (Tester.py:133-137), integers only ------------------------------------------
    long long s_true = 0, s_mt = 0, s_match = 0;
    for (int i = lane; i < N; i += kWave) {
        const long long lab = labels[beg + i];
        const long long p = (long long)flag[i];
        s_true += lab;
        s_match += lab == p ? 1 : 0;
        s_mt += (lab == p && p == 1) ? 1 : 0;
    }
    s_true = wave_sum(s_true);
    s_mt = wave_sum(s_mt);
    s_match = wave_sum(s_match);
    if (lane == 0) {
        nsel[d] = chosen;
        const long long c4[4] = {chosen, s_true, s_mt, s_match};
        for (int j = 0; j < 4; ++j) {
            doc_counts[4 * d + j] = (int32_t)c4[j];
            if (c4[j] != 0) atomicAdd(&totals[j], (unsigned long long)(long long)(int32_t)c4[j]);
        }
    }
}

}  // namespace

extern "C" {

int hsg_eval_select_supported(int n_max, int gram_max) {
    return n_max >= 1 && n_max <= kNMax && gram_max >= 0 && gram_max <= kGramMax;
}

int hsg_eval_select(int n, int B, const float *logits, const int64_t *labels, const int32_t *doc_off, int m,
                    int n_max, const int32_t *gram_ptr, const int32_t *gram_ids, const int32_t *gram_cnt,
                    int gram_max, int32_t *sel, int sel_ld, int32_t *nsel, int32_t *doc_counts, int64_t *totals,
                    void *stream) {
    if (n < 0 || B < 1 || m < 0 || !hsg_eval_select_supported(n_max, gram_max)) return HSG_EINVAL;
    if (sel_ld < (m == 0 ? n_max : (m < n_max ? m : n_max))) return HSG_EINVAL;
    if (!doc_off || !sel || !nsel || !doc_counts || !totals) return HSG_EINVAL;
    if (n > 0 && (!logits || !labels)) return HSG_EINVAL;
    if (gram_ptr && (!gram_ids || !gram_cnt)) return HSG_EINVAL;
    const bool blocking = m > 0 && gram_ptr;
    const size_t words = 3 * (size_t)n_max + (blocking ? ((size_t)gram_max + 31) / 32 : 0);
    hipLaunchKernelGGL(k_eval_select, dim3((unsigned)B), dim3(kWave), words * sizeof(uint32_t), (hipStream_t)stream, n,
                       logits, labels, doc_off, m, n_max, gram_ptr, gram_ids, gram_cnt, gram_max, sel, sel_ld, nsel,
                       doc_counts, reinterpret_cast<unsigned long long *>(totals));
    return status();
}

}  // extern "C"
