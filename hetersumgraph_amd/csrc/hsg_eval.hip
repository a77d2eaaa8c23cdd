// hsg_eval.hip -- the evaluation step's sentence selection (Tester.py:105-140, 155-184) for
// gfx950: per document the candidate order, top-m with or without n-gram blocking, the
// m == 0 argmax rule and the four match counters, in one launch per batch.
// C ABI and the whole contract: include/hsg_eval.h (blocking on dense n-gram ids made by the
// host) and include/hsg_eval_words.h (blocking on WORD ids, which depend neither on the window
// length nor on m: the device forms the n-gram windows itself).
//
// The work is tiny (32 to 256 documents of at most 50 rows in every BASELINE config); what
// the eager path pays for is host round trips, so the design is one launch and no read-back:
//
//   select_doc<Seen>     the one document body, for one block of ONE wave per document.  The
//                        scores become order-preserving integer keys in LDS; rank_i =
//                        #{j : key_j precedes key_i} by counting; the blocking walk is serial
//                        over the ranked candidates, the lanes striding over a candidate's
//                        n-grams, the verdict from a 64-bit ballot.  What "seen" means is the
//                        Seen type's: validate / clear / hits / room / insert.
//   k_eval_select        select_doc<GramSeen>: a bitmap over the document's dense n-gram ids,
//                        set with integer atomics; ids are validated before the walk.
//   k_eval_select_words  select_doc<WordSeen>: an open-addressing table; a slot holds the
//                        position in word_ids of a stored window's first word (-1: free),
//                        membership is decided by comparing the n_win ids, equal windows share
//                        a slot, slots are claimed with an integer compare-and-swap, every
//                        probe loop is bounded by tab_cap steps, and a document whose windows
//                        do not fit is refused during the walk.
//
// Dynamic LDS: key[n_max] | order[n_max] | flag[n_max] | bitmap[ceil(gram_max / 32)] or
// table[tab_cap], at most 12 KB + 32 KB.  A block is a single wave, so __syncthreads() orders
// its LDS traffic at the cost of a wait; all control flow around the barriers and ballots is
// wave-uniform (the probe loops of WordSeen diverge per lane, and hold neither).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_eval.h"
#include "../../include/hsg_eval_words.h"

namespace {

constexpr int kWave = 64;
constexpr int kNMax = 1024;
constexpr int kGramMax = 262144;
constexpr int kWinMax = 8;
constexpr int kTabMin = 64;
constexpr int kTabMax = 8192;

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

// ---- the two seen sets ---------------------------------------------------------------------
// Plain structs of the kernel's own arguments and the LDS tail.  select_doc reads ptr ([n + 1],
// NULL: no blocking) itself and clamps it: [lo, hi) is a candidate's (for validate: the
// document's) range in ids.  validate() and room() answer wave-uniformly, hits() per lane (the
// caller ballots); only GramSeen::validate, which the whole wave reaches, holds a ballot of
// its own, and none holds a barrier.

struct GramSeen {
    const int32_t *__restrict__ ptr, *__restrict__ ids, *__restrict__ cnt_of;
    int gram_max;
    uint32_t *bits;                                        // [ceil(gram_max / 32)]
    int cnt;                                               // set by validate()

    // gram_cnt in range and every id of the document below it
    __device__ __forceinline__ bool validate(int d, int lo, int hi, int lane) {
        cnt = cnt_of[d];
        if (cnt < 0 || cnt > gram_max) return false;
        bool bad = false;
        for (int t = lo + lane; t < hi; t += kWave) bad |= (uint32_t)ids[t] >= (uint32_t)cnt;
        return !__any(bad);
    }
    __device__ __forceinline__ void clear(int lane) const {
        for (int w = lane; w < (cnt + 31) / 32; w += kWave) bits[w] = 0u;
    }
    __device__ __forceinline__ bool hits(int lo, int hi, int lane) const {
        bool hit = false;
        for (int t = lo + lane; t < hi; t += kWave) {
            const uint32_t id = (uint32_t)ids[t];
            if (id < (uint32_t)cnt) hit |= (bits[id >> 5] >> (id & 31u)) & 1u;
        }
        return hit;
    }
    __device__ __forceinline__ bool room(int, int) const { return true; }
    __device__ __forceinline__ void insert(int lo, int hi, int lane) {
        for (int t = lo + lane; t < hi; t += kWave) {
            const uint32_t id = (uint32_t)ids[t];
            if (id < (uint32_t)cnt) atomicOr(&bits[id >> 5], 1u << (id & 31u));
        }
    }
};

// The hash only picks the first slot to look at: any function of the n_win ids is correct.
// Multiply-xorshift per id, so that ids that differ only in high bits (multiples of 4096) or
// only in bit 0 still spread over the table.
__device__ __forceinline__ uint32_t win_hash(const int32_t *__restrict__ w, int n_win) {
    uint32_t h = 0x811C9DC5u;
    for (int j = 0; j < n_win; ++j) {
        h = (h ^ (uint32_t)w[j]) * 0x9E3779B1u;
        h ^= h >> 15;
    }
    h *= 0x85EBCA6Bu;
    return h ^ (h >> 13);
}

__device__ __forceinline__ bool win_equal(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int n_win) {
    bool e = true;
    for (int j = 0; j < n_win; ++j) e &= a[j] == b[j];
    return e;
}

struct WordSeen {
    const int32_t *__restrict__ ptr, *__restrict__ ids;
    int n_win, tab_cap;
    int *tab;                                              // [tab_cap] first-word position, -1: free
    int stored;                                            // windows of the chosen sentences, with repeats

    // the windows of [lo, hi): window t reads ids[lo + t .. lo + t + n_win - 1] <= hi - 2
    __device__ __forceinline__ int windows(int lo, int hi) const { return hi - lo > n_win ? hi - lo - n_win : 0; }
    __device__ __forceinline__ bool validate(int, int, int, int) const { return true; }   // nothing to refuse
    __device__ __forceinline__ void clear(int lane) const {
        for (int s = lane; s < tab_cap; s += kWave) tab[s] = -1;
    }
    __device__ __forceinline__ bool hits(int lo, int hi, int lane) const {
        const int nw = windows(lo, hi);
        const uint32_t mask = (uint32_t)tab_cap - 1u;
        bool hit = false;
        for (int t = lane; t < nw && !hit; t += kWave) {
            const int32_t *w = ids + lo + t;
            uint32_t s = win_hash(w, n_win) & mask;
            for (int step = 0; step < tab_cap; ++step) {
                const int q = tab[s];
                if (q < 0) break;
                if (win_equal(ids + q, w, n_win)) {
                    hit = true;
                    break;
                }
                s = (s + 1u) & mask;
            }
        }
        return hit;
    }
    __device__ __forceinline__ bool room(int lo, int hi) const { return windows(lo, hi) <= tab_cap - stored; }
    __device__ __forceinline__ void insert(int lo, int hi, int lane) {
        const int nw = windows(lo, hi);
        const uint32_t mask = (uint32_t)tab_cap - 1u;
        for (int t = lane; t < nw; t += kWave) {
            const int p = lo + t;
            const int32_t *w = ids + p;
            uint32_t s = win_hash(w, n_win) & mask;
            // stored <= tab_cap slots are ever in use, so a free or an equal slot exists
            for (int step = 0; step < tab_cap; ++step) {
                const int q = atomicCAS(&tab[s], -1, p);
                if (q < 0 || win_equal(ids + q, w, n_win)) break;
                s = (s + 1u) & mask;
            }
        }
        stored += nw;
    }
};

// ---- one document ----------------------------------------------------------------------------
template <class Seen>
__device__ __forceinline__ void select_doc(uint32_t *lds, int n, const float *__restrict__ logits,
                                           const int64_t *__restrict__ labels, const int32_t *__restrict__ doc_off,
                                           int m, int n_max, Seen seen, int32_t *__restrict__ sel, int sel_ld,
                                           int32_t *__restrict__ nsel, int32_t *__restrict__ doc_counts,
                                           unsigned long long *__restrict__ totals) {
    uint32_t *key = lds;                                   // [n_max]
    int32_t *order = reinterpret_cast<int32_t *>(lds + n_max);      // [n_max] rank -> local index
    uint32_t *flag = lds + 2 * n_max;                      // [n_max] 1: selected

    const int d = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int beg = clampi(doc_off[d], 0, n);
    const int end = clampi(doc_off[d + 1], beg, n);
    const int N = end - beg;
    int32_t *srow = sel + (size_t)d * sel_ld;
    const bool blocking = m > 0 && seen.ptr != nullptr;

    bool refused = N > n_max;                              // wave-uniform, here and below
    if (!refused && blocking) {
        const int T = seen.ptr[n] < 0 ? 0 : seen.ptr[n];
        const int lo = clampi(seen.ptr[beg], 0, T);
        refused = !seen.validate(d, lo, clampi(seen.ptr[end], lo, T), lane);
    }
    int chosen = 0;
    if (!refused && m == 0) {
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
    } else if (!refused) {
        const int k = m < N ? m : N;
        for (int i = lane; i < N; i += kWave) {
            key[i] = score_key(logits[2 * (size_t)(beg + i) + 1]);
            flag[i] = 0u;
        }
        if (blocking) seen.clear(lane);
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
            // T is read again, not kept live across the ranking: k_eval_select_words sits at the
            // 100 SGPRs beyond which a SIMD holds 7 waves instead of 8.
            const int T = seen.ptr[n] < 0 ? 0 : seen.ptr[n];
            for (int c = 0; c < N && chosen < k; ++c) {
                const int i = order[c];
                const int lo = clampi(seen.ptr[beg + i], 0, T);
                const int hi = clampi(seen.ptr[beg + i + 1], lo, T);
                if (__any(seen.hits(lo, hi, lane))) continue;   // wave-uniform
                if (!seen.room(lo, hi)) {                  // checked before anything is inserted
                    refused = true;
                    break;
                }
                __syncthreads();                           // every lane tested before anything is inserted
                seen.insert(lo, hi, lane);
                // The lane that would pad this column writes it: a later refusal's -1 fill of the
                // column then comes from the same lane and wins by program order.
                if (lane == (chosen & (kWave - 1))) srow[chosen] = i;
                if (lane == 0) flag[i] = 1u;
                ++chosen;
                __syncthreads();                           // the insertions are visible to the next candidate
            }
        }
    }
    if (refused) {
        for (int c = lane; c < sel_ld; c += kWave) srow[c] = -1;
        if (lane == 0) nsel[d] = -1;
        if (lane < 4) doc_counts[4 * d + lane] = 0;
        return;
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

__global__ __launch_bounds__(kWave) void k_eval_select(
    int n, const float *__restrict__ logits, const int64_t *__restrict__ labels, const int32_t *__restrict__ doc_off,
    int m, int n_max, const int32_t *__restrict__ gram_ptr, const int32_t *__restrict__ gram_ids,
    const int32_t *__restrict__ gram_cnt, int gram_max, int32_t *__restrict__ sel, int sel_ld,
    int32_t *__restrict__ nsel, int32_t *__restrict__ doc_counts, unsigned long long *__restrict__ totals) {
    extern __shared__ uint32_t lds[];
    const GramSeen seen{gram_ptr, gram_ids, gram_cnt, gram_max, lds + 3 * n_max, 0};
    select_doc(lds, n, logits, labels, doc_off, m, n_max, seen, sel, sel_ld, nsel, doc_counts, totals);
}

__global__ __launch_bounds__(kWave) void k_eval_select_words(
    int n, const float *__restrict__ logits, const int64_t *__restrict__ labels, const int32_t *__restrict__ doc_off,
    int m, int n_max, int n_win, const int32_t *__restrict__ word_ptr, const int32_t *__restrict__ word_ids,
    int tab_cap, int32_t *__restrict__ sel, int sel_ld, int32_t *__restrict__ nsel, int32_t *__restrict__ doc_counts,
    unsigned long long *__restrict__ totals) {
    extern __shared__ uint32_t lds[];
    const WordSeen seen{word_ptr, word_ids, n_win, tab_cap, reinterpret_cast<int *>(lds + 3 * n_max), 0};
    select_doc(lds, n, logits, labels, doc_off, m, n_max, seen, sel, sel_ld, nsel, doc_counts, totals);
}

// The argument checks both entry points share (n_max is already within 1..kNMax).
bool args_ok(int n, int B, const void *logits, const void *labels, const void *doc_off, int m, int n_max,
             const void *sel, int sel_ld, const void *nsel, const void *doc_counts, const void *totals) {
    if (n < 0 || B < 1 || m < 0) return false;
    if (sel_ld < (m == 0 ? n_max : (m < n_max ? m : n_max))) return false;
    if (!doc_off || !sel || !nsel || !doc_counts || !totals) return false;
    return n == 0 || (logits && labels);
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
    if (!hsg_eval_select_supported(n_max, gram_max) ||
        !args_ok(n, B, logits, labels, doc_off, m, n_max, sel, sel_ld, nsel, doc_counts, totals))
        return HSG_EINVAL;
    if (gram_ptr && (!gram_ids || !gram_cnt)) return HSG_EINVAL;
    const bool blocking = m > 0 && gram_ptr;
    const size_t words = 3 * (size_t)n_max + (blocking ? ((size_t)gram_max + 31) / 32 : 0);
    hipLaunchKernelGGL(k_eval_select, dim3((unsigned)B), dim3(kWave), words * sizeof(uint32_t), (hipStream_t)stream, n,
                       logits, labels, doc_off, m, n_max, gram_ptr, gram_ids, gram_cnt, gram_max, sel, sel_ld, nsel,
                       doc_counts, reinterpret_cast<unsigned long long *>(totals));
    return status();
}

int hsg_eval_words_supported(int n_max, int n_win, int tab_cap) {
    return n_max >= 1 && n_max <= kNMax && n_win >= 1 && n_win <= kWinMax && tab_cap >= kTabMin &&
           tab_cap <= kTabMax && (tab_cap & (tab_cap - 1)) == 0;
}

int hsg_eval_select_words(int n, int B, const float *logits, const int64_t *labels, const int32_t *doc_off, int m,
                          int n_max, int n_win, const int32_t *word_ptr, const int32_t *word_ids, int tab_cap,
                          int32_t *sel, int sel_ld, int32_t *nsel, int32_t *doc_counts, int64_t *totals,
                          void *stream) {
    if (!hsg_eval_words_supported(n_max, n_win, tab_cap) ||
        !args_ok(n, B, logits, labels, doc_off, m, n_max, sel, sel_ld, nsel, doc_counts, totals))
        return HSG_EINVAL;
    if (word_ptr && !word_ids) return HSG_EINVAL;
    const bool blocking = m > 0 && word_ptr;
    const size_t words = 3 * (size_t)n_max + (blocking ? (size_t)tab_cap : 0);
    hipLaunchKernelGGL(k_eval_select_words, dim3((unsigned)B), dim3(kWave), words * sizeof(uint32_t),
                       (hipStream_t)stream, n, logits, labels, doc_off, m, n_max, n_win, word_ptr, word_ids, tab_cap,
                       sel, sel_ld, nsel, doc_counts, reinterpret_cast<unsigned long long *>(totals));
    return status();
}

}  // extern "C"
