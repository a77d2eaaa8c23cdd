// hsg_resident_eval.hip -- the eval view of a resident batch for gfx950.
// C ABI and the whole contract: include/hsg_resident_eval.h.
//
// The word pack of the native evaluation step, [word_ptr (n_sent + 1) | word_ids (n_words)], is
// per document a stored row end plus the batch's running word offset, and the stored ids copied.
// One launch, a flat grid over the n_sent + n_words output elements behind pack[0]: an element
// finds its document by a binary search over the B + 1 running offsets of its family (offs[SENT]
// for a row end, wordbase for an id), so a document of thousands of words spreads over as many
// blocks as its words need and neighbouring lanes read neighbouring stored elements.  The search
// reads at most 20 cached words per element (B <= 2^20; 5 at B = 32) against one gathered int32.
//
// Each thread owns the output elements it writes and every index comes from the search, so an
// element is written at most once and never outside [0, its count) whatever the offsets hold; a
// stored element is read only after its index was checked against the document's own count.
// Pure integer adds and copies: nothing is accumulated, so the result cannot depend on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_resident_eval.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = 1 << 16;
constexpr int kMaxB = 1 << 20;
constexpr int64_t kMaxCount = 2147483647LL;

struct Args {
    int64_t n_docs;
    const int64_t *sstart;          // hsg_res_store's starts[HSG_RES_SENT]: [n_docs + 1]
    hsg_res_eval_cols c;
    int B;
    const int32_t *pick;
    const int64_t *soff;            // offs[HSG_RES_SENT]: [B + 1]
    const int32_t *wordbase;        // [B + 1]
    int64_t n_sent, n_words;
    int32_t *pack;
};

// the last d in [0, B) with off[d] <= e (d = 0 when there is none): the document that holds
// element e when off is non-decreasing from 0; only off[1 .. B-1] is read
template <typename T>
__device__ inline int doc_of(const T *__restrict__ off, int B, int64_t e) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void k_res_eval(Args a) {
    const int64_t total = a.n_sent + a.n_words;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t0 == 0) {
        a.pack[0] = 0;
        if (a.n_words == 0) a.pack[a.n_sent + 1] = 0;          // the padding element
    }
    for (int64_t e = t0; e < total; e += (int64_t)gridDim.x * kThreads) {
        if (e < a.n_sent) {                                    // a row end
            const int d = doc_of(a.soff, a.B, e);
            const uint32_t s = (uint32_t)a.pick[d];
            if ((int64_t)s >= a.n_docs) continue;
            const int64_t i = e - a.soff[d], s0 = a.sstart[s];
            if ((uint64_t)i >= (uint64_t)(a.sstart[s + 1] - s0)) continue;
            const int64_t W = a.c.wstart[s + 1] - a.c.wstart[s];
            int64_t end = a.c.wend[s0 + i];
            end = end < 0 ? 0 : end > W ? W : end;
            a.pack[1 + e] = (int32_t)((int64_t)a.wordbase[d] + end);
        } else {                                               // a word id
            const int64_t k = e - a.n_sent;
            const int d = doc_of(a.wordbase, a.B, k);
            const uint32_t s = (uint32_t)a.pick[d];
            if ((int64_t)s >= a.n_docs) continue;
            const int64_t i = k - (int64_t)a.wordbase[d], w0 = a.c.wstart[s];
            if ((uint64_t)i >= (uint64_t)(a.c.wstart[s + 1] - w0)) continue;
            a.pack[a.n_sent + 1 + k] = a.c.wid[w0 + i];
        }
    }
}

}  // namespace

extern "C" int hsg_res_eval_supported(int B, int64_t n_sent, int64_t n_words) {
    if (B < 1 || B > kMaxB || n_sent < 0 || n_words < 0 || n_sent > kMaxCount || n_words > kMaxCount) return 0;
    return n_sent + 1 + (n_words > 1 ? n_words : 1) <= kMaxCount;
}

extern "C" int hsg_res_eval(const hsg_res_store *st, const hsg_res_eval_cols *cols, int B, const int32_t *pick,
                            const int64_t *offs, const int32_t *wordbase, int64_t n_sent, int64_t n_words,
                            int32_t *pack, void *stream) {
    if (!st || !pick || !st->starts || !st->bases || st->n_docs < 1 || st->n_docs > kMaxCount) return HSG_EINVAL;
    if (B < 1 || B > kMaxB || !cols || !offs || !wordbase || !pack || !cols->wstart) return HSG_EINVAL;
    if (!hsg_res_eval_supported(B, n_sent, n_words)) return HSG_EINVAL;
    if ((n_sent > 0 && !cols->wend) || (n_words > 0 && !cols->wid)) return HSG_EINVAL;
    Args a{st->n_docs, st->starts + (int64_t)HSG_RES_SENT * (st->n_docs + 1), *cols, B, pick,
           offs + (int64_t)HSG_RES_SENT * ((int64_t)B + 1), wordbase, n_sent, n_words, pack};
    const int64_t total = n_sent + n_words;
    const int64_t blocks = total > 0 ? (total + kThreads - 1) / kThreads : 1;
    k_res_eval<<<dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), kThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
