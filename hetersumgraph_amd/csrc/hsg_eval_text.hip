// hsg_eval_text.hip -- document-local word ids from the sentences' UTF-8 bytes, for gfx950: the
// blocking operand of hsg_eval_select_words (hsg_eval.hip) made on the device, so that
// the host neither splits nor interns.  C ABI and the whole contract: include/hsg_eval_text.h.
//
//   k_text_count   one wave per row.  Lane j of a stride looks at byte p = lo + base + j: a
//                  word starts at p iff no whitespace sequence covers p and p is the row's
//                  first byte or p - 1 is covered.  "Covered" depends on the sequences that
//                  start at p, p - 1 and p - 2 only, all read inside [lo, hi).  The row's count
//                  is the popcount of the 64-bit ballots; it is left in word_ptr[i + 1].
//   k_text_scan    one block.  word_ptr becomes the inclusive sum of the counts, capped at the
//                  bound; doc_row[d] = e_d, the running maximum of the clamped inner doc_off.
//   k_text_emit    one wave per row, the same predicate: the word of rank r in the row is
//                  position k = word_ptr[i] + r; its first byte and its length (a serial scan
//                  to the next sequence start, words are short) go to ws.
//   k_text_intern  one block per document, a thread per word.  The document's table is the
//                  slice [2 * w0, 2 * w1) of ws's slots, w0 .. w1 being its word positions: a
//                  load of one half.  The block clears it, then every word probes linearly
//                  from its hash: an empty slot is claimed with atomicCAS, a slot whose
//                  representative has the same bytes is lowered with atomicMin; the slot's
//                  index is parked in word_ids[k].  Slots are never freed and equal words walk
//                  the same probe sequence, so equal words end in the same slot.  After a
//                  barrier word_ids[k] = the slot's final value, the smallest equal position.
//                  The words' first bytes and lengths were written by the launch before, so a
//                  representative's bytes are visible whichever wave published it.
//
// The table is read and written with atomics only while it is probed (device scope, at L2), so
// no wave sees a stale slot through its L1.  Integer atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_eval_text.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowBlock = 256;                             // 4 rows per block
constexpr int kScanBlock = 1024;
constexpr int kDocBlock = 1024;
constexpr int kRowsMax = 1 << 20;
constexpr int kDocsMax = 1 << 20;
constexpr int64_t kBytesMax = (int64_t)1 << 30;
constexpr int kEmpty = 0x7FFFFFFF;

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Length of the whitespace sequence that starts at byte p of a row that ends at hi (p < hi),
// 0 if none does.  Reads t[p .. min(p + 3, hi)) only.
__device__ __forceinline__ int ws_len(const uint8_t *__restrict__ t, int p, int hi) {
    const uint32_t b0 = t[p];
    if (b0 <= 0x20u) return ((b0 >= 0x09u && b0 <= 0x0Du) || b0 >= 0x1Cu) ? 1 : 0;
    if (b0 == 0xC2u) {
        if (p + 1 >= hi) return 0;
        const uint32_t b1 = t[p + 1];
        return (b1 == 0x85u || b1 == 0xA0u) ? 2 : 0;
    }
    if (b0 < 0xE1u || b0 > 0xE3u || p + 2 >= hi) return 0;
    const uint32_t b1 = t[p + 1], b2 = t[p + 2];
    if (b0 == 0xE1u) return (b1 == 0x9Au && b2 == 0x80u) ? 3 : 0;
    if (b0 == 0xE3u) return (b1 == 0x80u && b2 == 0x80u) ? 3 : 0;
    if (b1 == 0x80u) return ((b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu) ? 3 : 0;
    return (b1 == 0x81u && b2 == 0x9Fu) ? 3 : 0;
}

// Does a word start at byte p of the row [lo, hi)?  lo <= p < hi.
__device__ __forceinline__ bool word_starts(const uint8_t *__restrict__ t, int p, int lo, int hi) {
    const int l0 = ws_len(t, p, hi);
    const int l1 = p - 1 >= lo ? ws_len(t, p - 1, hi) : 0;
    const int l2 = p - 2 >= lo ? ws_len(t, p - 2, hi) : 0;
    const int l3 = p - 3 >= lo ? ws_len(t, p - 3, hi) : 0;
    const bool here = l0 >= 1 || l1 >= 2 || l2 >= 3;
    const bool before = p == lo || l1 >= 1 || l2 >= 2 || l3 >= 3;
    return !here && before;
}

__global__ __launch_bounds__(kRowBlock) void k_text_count(int n, const uint8_t *__restrict__ text, int nbytes,
                                                          const int32_t *__restrict__ byte_ptr,
                                                          int32_t *__restrict__ word_ptr) {
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int i = (int)blockIdx.x * (kRowBlock / kWave) + ((int)threadIdx.x >> 6);   // wave-uniform
    if (i >= n) return;
    const int lo = clampi(byte_ptr[i], 0, nbytes);
    const int hi = clampi(byte_ptr[i + 1], lo, nbytes);
    int cnt = 0;
    for (int base = lo; base < hi; base += kWave) {
        const int p = base + lane;
        const bool st = p < hi && word_starts(text, p, lo, hi);
        cnt += __popcll(__ballot(st));
    }
    if (lane == 0) word_ptr[i + 1] = cnt;
}

// Inclusive scan of one value per thread over the block, `carry` added; returns this thread's
// inclusive value, and the block's total (carry included) in *total.  MAX: running maximum.
template <bool MAX>
__device__ __forceinline__ long long block_scan(long long v, long long carry, long long *wsum, long long *total) {
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const long long o = __shfl_up(v, off, kWave);
        if (lane >= off) v = MAX ? (o > v ? o : v) : v + o;
    }
    if (lane == kWave - 1) wsum[wave] = v;
    __syncthreads();
    long long pre = carry;
    for (int w = 0; w < wave; ++w) pre = MAX ? (wsum[w] > pre ? wsum[w] : pre) : pre + wsum[w];
    long long tot = carry;
    for (int w = 0; w < kScanBlock / kWave; ++w) tot = MAX ? (wsum[w] > tot ? wsum[w] : tot) : tot + wsum[w];
    __syncthreads();                                       // wsum is reused by the next chunk
    *total = tot;
    return MAX ? (pre > v ? pre : v) : pre + v;
}

__global__ __launch_bounds__(kScanBlock) void k_text_scan(int n, int B, int bound, const int32_t *__restrict__ doc_off,
                                                          int32_t *__restrict__ word_ptr,
                                                          int32_t *__restrict__ doc_row) {
    __shared__ long long wsum[kScanBlock / kWave];
    const int t = (int)threadIdx.x;
    long long carry = 0;
    if (t == 0) word_ptr[0] = 0;
    for (int base = 0; base < n; base += kScanBlock) {     // block-uniform trip count
        const int i = base + t;
        const long long c = i < n ? (long long)word_ptr[i + 1] : 0;
        long long total;
        const long long s = block_scan<false>(c, carry, wsum, &total);
        if (i < n) word_ptr[i + 1] = (int32_t)(s < (long long)bound ? s : (long long)bound);
        carry = total;
    }
    // doc_row[0] = 0, doc_row[d] = max(doc_row[d - 1], clamp(doc_off[d], 0, n)) for 0 < d < B, doc_row[B] = n
    carry = 0;
    for (int base = 0; base <= B; base += kScanBlock) {
        const int d = base + t;
        const long long c = (d > 0 && d < B) ? (long long)clampi(doc_off[d], 0, n) : 0;
        long long total;
        const long long s = block_scan<true>(c, carry, wsum, &total);
        if (d < B) doc_row[d] = (int32_t)s;
        else if (d == B) doc_row[d] = n;
        carry = total;
    }
}

__global__ __launch_bounds__(kRowBlock) void k_text_emit(int n, const uint8_t *__restrict__ text, int nbytes,
                                                         const int32_t *__restrict__ byte_ptr,
                                                         const int32_t *__restrict__ word_ptr,
                                                         int32_t *__restrict__ w_first, int32_t *__restrict__ w_len) {
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int i = (int)blockIdx.x * (kRowBlock / kWave) + ((int)threadIdx.x >> 6);   // wave-uniform
    if (i >= n) return;
    const int lo = clampi(byte_ptr[i], 0, nbytes);
    const int hi = clampi(byte_ptr[i + 1], lo, nbytes);
    const int k0 = word_ptr[i], k1 = word_ptr[i + 1];      // capped at the bound: k < k1 is in ws
    int rank = 0;
    for (int base = lo; base < hi; base += kWave) {
        const int p = base + lane;
        const bool st = p < hi && word_starts(text, p, lo, hi);
        const unsigned long long mask = __ballot(st);
        const int k = k0 + rank + __popcll(mask & ((1ull << lane) - 1ull));
        if (st && k < k1) {
            int q = p + 1;                                 // the word ends where the next sequence starts
            while (q < hi && ws_len(text, q, hi) == 0) ++q;
            w_first[k] = p;
            w_len[k] = q - p;
        }
        rank += __popcll(mask);
    }
}

// The hash only picks the first slot to look at: any function of the bytes is correct.
__device__ __forceinline__ uint32_t bytes_hash(const uint8_t *__restrict__ s, int len) {
    uint32_t h = 0x811C9DC5u ^ (uint32_t)len;
    for (int j = 0; j < len; ++j) h = (h ^ (uint32_t)s[j]) * 0x01000193u;
    h ^= h >> 15;
    h *= 0x85EBCA6Bu;
    return h ^ (h >> 13);
}

__device__ __forceinline__ bool bytes_equal(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int len) {
    for (int j = 0; j < len; ++j)
        if (a[j] != b[j]) return false;
    return true;
}

__global__ __launch_bounds__(kDocBlock) void k_text_intern(const uint8_t *__restrict__ text,
                                                           const int32_t *__restrict__ word_ptr,
                                                           const int32_t *__restrict__ doc_row,
                                                           const int32_t *__restrict__ w_first,
                                                           const int32_t *__restrict__ w_len, int *__restrict__ slots,
                                                           int32_t *__restrict__ word_ids) {
    const int d = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int w0 = word_ptr[doc_row[d]], w1 = word_ptr[doc_row[d + 1]];   // ascending: word_ptr is a capped sum
    const int W = w1 - w0;                                 // block-uniform
    if (W <= 0) return;
    int *tab = slots + 2 * (size_t)w0;                     // [2 * W], inside the 2 * bound slots
    const uint32_t size = 2u * (uint32_t)W;
    for (uint32_t s = (uint32_t)t; s < size; s += kDocBlock)
        __hip_atomic_store(&tab[s], kEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __syncthreads();
    for (int k = w0 + t; k < w1; k += kDocBlock) {
        const int len = w_len[k];
        const uint8_t *w = text + w_first[k];
        uint32_t s = (uint32_t)(((uint64_t)bytes_hash(w, len) * size) >> 32);
        int slot = (int)s;
        for (uint32_t step = 0; step < size; ++step) {     // at most W slots are ever in use: one is free or equal
            int q = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (q == kEmpty) q = atomicCAS(&tab[s], kEmpty, k);
            if (q == kEmpty) {
                slot = (int)s;
                break;
            }
            if (w_len[q] == len && bytes_equal(text + w_first[q], w, len)) {   // w0 <= q < w1: a word of this document
                atomicMin(&tab[s], k);
                slot = (int)s;
                break;
            }
            s = s + 1u == size ? 0u : s + 1u;
        }
        word_ids[k] = slot;                                // read back by this thread below
    }
    __threadfence();
    __syncthreads();
    for (int k = w0 + t; k < w1; k += kDocBlock)
        word_ids[k] = __hip_atomic_load(&tab[word_ids[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" {

int hsg_eval_text_supported(int n, int B, int64_t nbytes) {
    return n >= 0 && n <= kRowsMax && B >= 1 && B <= kDocsMax && nbytes >= 0 && nbytes <= kBytesMax;
}

int64_t hsg_eval_text_word_bound(int n, int64_t nbytes) {
    return hsg_eval_text_supported(n, 1, nbytes) ? (nbytes + n) / 2 : 0;
}

size_t hsg_eval_text_workspace_bytes(int n, int B, int64_t nbytes) {
    if (!hsg_eval_text_supported(n, B, nbytes)) return 0;
    return sizeof(int32_t) * (4 * (size_t)hsg_eval_text_word_bound(n, nbytes) + (size_t)B + 1);
}

int hsg_eval_text_words(int n, int B, const uint8_t *text, int64_t nbytes, const int32_t *byte_ptr,
                        const int32_t *doc_off, int64_t word_cap, int32_t *word_ptr, int32_t *word_ids, void *ws,
                        void *stream) {
    if (!hsg_eval_text_supported(n, B, nbytes)) return HSG_EINVAL;
    const int64_t bound = hsg_eval_text_word_bound(n, nbytes);
    if (word_cap < bound) return HSG_EINVAL;
    if (!byte_ptr || !doc_off || !word_ptr || !ws) return HSG_EINVAL;
    if ((nbytes > 0 && !text) || (bound > 0 && !word_ids)) return HSG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int32_t *w_first = static_cast<int32_t *>(ws);         // [bound]
    int32_t *w_len = w_first + bound;                      // [bound]
    int32_t *slots = w_len + bound;                        // [2 * bound]
    int32_t *doc_row = slots + 2 * bound;                  // [B + 1]
    const unsigned row_blocks = (unsigned)((n + kRowBlock / kWave - 1) / (kRowBlock / kWave));
    if (n > 0)
        hipLaunchKernelGGL(k_text_count, dim3(row_blocks), dim3(kRowBlock), 0, st, n, text, (int)nbytes, byte_ptr,
                           word_ptr);
    hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(kScanBlock), 0, st, n, B, (int)bound, doc_off, word_ptr, doc_row);
    if (n > 0 && bound > 0) {
        hipLaunchKernelGGL(k_text_emit, dim3(row_blocks), dim3(kRowBlock), 0, st, n, text, (int)nbytes, byte_ptr,
                           word_ptr, w_first, w_len);
        hipLaunchKernelGGL(k_text_intern, dim3((unsigned)B), dim3(kDocBlock), 0, st, text, word_ptr, doc_row, w_first,
                           w_len, slots, word_ids);
    }
    return status();
}

}  // extern "C"
