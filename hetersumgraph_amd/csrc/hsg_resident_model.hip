// hsg_resident_model.hip -- the model view of a resident batch for gfx950.
// C ABI and the whole contract: include/hsg_resident_model.h.
//
// What the model derives from a batch before its first kernel -- the sentence node list, the
// sentences' token rows, lengths and CNN row offsets, the LSTM's document offsets and previous
// rows, the tf-idf table index -- is a function of the picked documents and the running offsets
// of hsg_res_offsets, like the batch itself.  One launch, blockIdx.y the job:
//
//   kNodes   walks a document's nodes: a node with a sentence rank writes its batch id at the
//            rank's row of sent_nodes.
//   kRows    walks a document's sentence rows, a wave per row: the token row widened, and from
//            lane 0 the row's position, length, row offset and previous rows.
//   kEdges   walks a document's edges: the tf-idf index.
//   kDocs    walks the B + 1 document offsets: doc_off, and the closing element of rowoff.
//
// blockIdx.x walks (document, part) units as k_res_gather does.  Pure integer copies: nothing
// is accumulated, so the result cannot depend on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_resident_model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kParts = 8;           // runs per document (fewer once B alone fills the device)
constexpr int kMaxBlocksX = 4096;
constexpr int kMaxB = 1 << 20;
constexpr int64_t kMaxCount = 2147483647LL;

enum Job : int { kNodes = 0, kRows, kEdges, kDocs, kJobs };

struct Args {
    int64_t n_docs;
    const int64_t *starts, *bases;
    const int32_t *sent_rank, *words, *tok_len, *tok_row;
    const uint8_t *tffrac, *edtype;
    int width, B;
    const int32_t *pick;
    const int64_t *offs;
    const int32_t *rowbase;
    int64_t n_sent, n_edges;
    int64_t *sent_nodes, *sent_ids, *sent_pos, *sent_len;
    int32_t *rowoff, *doc_off;
    int64_t *prev, *tfidf_index;
};

__global__ __launch_bounds__(kThreads) void k_res_model(Args a, int parts) {
    const int job = blockIdx.y;
    const int64_t B1 = (int64_t)a.B + 1;
    if (job == kDocs) {
        const int64_t *so = a.offs + HSG_RES_SENT * B1;
        for (int64_t d = (int64_t)blockIdx.x * kThreads + threadIdx.x; d < B1; d += (int64_t)gridDim.x * kThreads)
            a.doc_off[d] = (int32_t)so[d];
        if (blockIdx.x == 0 && threadIdx.x == 0) a.rowoff[a.n_sent] = a.rowbase[a.B];
        return;
    }
    const int fam = job == kNodes ? HSG_RES_NODE : job == kRows ? HSG_RES_SENT : HSG_RES_EDGE;
    const int64_t *st = a.starts + (int64_t)fam * (a.n_docs + 1);
    const int64_t *ss = a.starts + (int64_t)HSG_RES_SENT * (a.n_docs + 1);
    const int64_t units = (int64_t)a.B * parts;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int d = (int)(u / parts), p = (int)(u % parts);
        const uint32_t s = (uint32_t)a.pick[d];
        if ((int64_t)s >= a.n_docs) continue;
        const int64_t s0 = st[s], cnt = st[s + 1] - s0;
        const int64_t lo = cnt / parts * p + min((int64_t)p, cnt % parts);
        const int64_t hi = lo + cnt / parts + (p < cnt % parts ? 1 : 0);
        if (lo >= hi) continue;
        const int64_t o0 = a.offs[fam * B1 + d];
        if (job == kNodes) {
            const int64_t rows = ss[s + 1] - ss[s], g0 = a.offs[HSG_RES_SENT * B1 + d];
            for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
                const uint32_t r = (uint32_t)a.sent_rank[s0 + i];
                if ((int64_t)r < rows && g0 + r < a.n_sent) a.sent_nodes[g0 + r] = o0 + i;
            }
        } else if (job == kRows) {
            const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
            const int64_t base = a.rowbase[d];
            for (int64_t r = lo + wave; r < hi; r += kThreads / kWave) {
                const int64_t g = o0 + r;
                if (g >= a.n_sent) continue;
                const int32_t *src = a.words + (s0 + r) * a.width;
                int64_t *dst = a.sent_ids + g * a.width;
                for (int c = lane; c < a.width; c += kWave) dst[c] = (int64_t)src[c];
                if (lane == 0) {
                    a.sent_pos[g] = r + 1;
                    a.sent_len[g] = (int64_t)a.tok_len[s0 + r];
                    a.rowoff[g] = (int32_t)(base + a.tok_row[s0 + r]);
                    a.prev[2 * g] = r > 0 ? g - 1 : a.n_sent;
                    a.prev[2 * g + 1] = r < cnt - 1 ? g + 1 : a.n_sent;
                }
            }
        } else {
            for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
                const int64_t o = o0 + j;
                if (o < a.n_edges) a.tfidf_index[o] = a.edtype[s0 + j] == 0 ? (int64_t)a.tffrac[s0 + j] : -1;
            }
        }
    }
}

}  // namespace

extern "C" int hsg_res_model_supported(int B, int64_t n_sent, int64_t n_edges, int64_t n_rows) {
    return hsg_res_supported(B, n_sent, n_edges, 0) && n_rows >= 0 && n_rows <= kMaxCount;
}

extern "C" int hsg_res_model(const hsg_res_store *st, const int32_t *tok_len, const int32_t *tok_row, int B,
                             const int32_t *pick, const int64_t *offs, const int32_t *rowbase, int64_t n_sent,
                             int64_t n_edges, int64_t *sent_nodes, int64_t *sent_ids, int64_t *sent_pos,
                             int64_t *sent_len, int32_t *rowoff, int32_t *doc_off, int64_t *prev,
                             int64_t *tfidf_index, void *stream) {
    if (!st || !pick || !st->starts || !st->bases || st->n_docs < 1 || st->n_docs > kMaxCount) return HSG_EINVAL;
    if (B < 1 || B > kMaxB || !offs || !rowbase || st->sent_len < 1) return HSG_EINVAL;
    if (!hsg_res_model_supported(B, n_sent, n_edges, 0) || !rowoff || !doc_off) return HSG_EINVAL;
    if (n_sent > 0 && (!sent_nodes || !sent_ids || !sent_pos || !sent_len || !prev || !tok_len || !tok_row ||
                       !st->sent_rank || !st->words))
        return HSG_EINVAL;
    if (n_edges > 0 && (!tfidf_index || !st->tffrac || !st->edtype)) return HSG_EINVAL;
    Args a{st->n_docs, st->starts, st->bases, st->sent_rank, st->words, tok_len, tok_row, st->tffrac, st->edtype,
           st->sent_len, B, pick, offs, rowbase, n_sent, n_edges, sent_nodes, sent_ids, sent_pos, sent_len, rowoff,
           doc_off, prev, tfidf_index};
    const int parts = B >= kMaxBlocksX / kParts ? 1 : kParts;
    const int64_t units = (int64_t)B * parts;
    dim3 grid((unsigned)(units < kMaxBlocksX ? units : kMaxBlocksX), (unsigned)kJobs);
    k_res_model<<<grid, kThreads, 0, (hipStream_t)stream>>>(a, parts);
    return (int)hipGetLastError();
}
