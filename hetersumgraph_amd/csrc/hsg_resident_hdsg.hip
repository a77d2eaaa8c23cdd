// hsg_resident_hdsg.hip -- the doc view of a resident batch for gfx950.
// C ABI and the whole contract: include/hsg_resident_hdsg.h.
//
// What HSumDocGraph builds on the host from a multi-document batch -- the sentence -> doc pair
// list, the supernode order, the per-sentence supernode rows, the pair list's CSR / CSC forms
// and the inverse supernode lists of the native glue -- is, per document, a stored local value
// plus a running offset of its family.  One launch, blockIdx.y the family:
//
//   kPair   a document's sentence -> doc pairs: pair_s, pair_d, doc_sent, sent_doc.
//   kSent   its sentences: sent_super, doc_super (both widths), sent_ptr, sent_row, sup_list.
//   kDocn   its doc nodes: inv_cnt (copied), doc_ptr, doc_row.
//   kSup    its supernodes: super_pos, super_src, sup_sent, sup_ptr.
//
// blockIdx.x walks the documents (a document holds tens of elements of each family, so a block
// per document and family is the whole launch at the batch sizes the model trains on).  The
// closing elements of the three pointer arrays come from the block (0, family) that owns them.
// Pure integer adds and copies: nothing is accumulated, so the result cannot depend on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_resident_hdsg.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 4096;
constexpr int kMaxB = 1 << 20;
constexpr int64_t kMaxCount = 2147483647LL;

enum Job : int { kPair = 0, kSent, kDocn, kSup, kJobs };

struct Args {
    int64_t n_docs;
    const int64_t *starts;          // hsg_res_store's [NFAM][n_docs + 1]
    hsg_res_hdsg_cols c;
    int B;
    const int32_t *pick;
    const int64_t *offs;
    const int32_t *docbase, *pairbase;
    int64_t n_sent, n_docn, n_pair, n_super;
    int64_t *pair_s, *pair_d, *super_pos, *sent_super64, *doc_super64;
    float *inv_cnt;
    int32_t *super_src, *doc_ptr, *doc_sent, *sent_ptr, *sent_doc, *sent_row, *doc_row, *sent_super, *doc_super,
        *sup_sent, *sup_ptr, *sup_list;
};

// an output index inside [0, limit): a negative or oversized offset writes nothing
__device__ inline bool inside(int64_t o, int64_t limit) { return (uint64_t)o < (uint64_t)limit; }

__global__ __launch_bounds__(kThreads) void k_res_hdsg(Args a) {
    const int job = blockIdx.y;
    const int64_t B1 = (int64_t)a.B + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {                 // the closing elements
        if (job == kDocn) a.doc_ptr[a.n_docn] = (int32_t)a.n_pair;
        if (job == kSent) a.sent_ptr[a.n_sent] = (int32_t)a.n_pair;
        if (job == kSup) a.sup_ptr[a.n_super] = (int32_t)a.n_sent;
    }
    const int64_t *st = job == kPair   ? a.c.pstart
                        : job == kDocn ? a.c.dstart
                        : a.starts + (int64_t)(job == kSent ? HSG_RES_SENT : HSG_RES_DST(0)) * (a.n_docs + 1);
    for (int64_t d = blockIdx.x; d < a.B; d += gridDim.x) {
        const uint32_t s = (uint32_t)a.pick[d];
        if ((int64_t)s >= a.n_docs) continue;
        const int64_t s0 = st[s], cnt = st[s + 1] - s0;
        const int64_t so = a.offs[HSG_RES_SENT * B1 + d], uo = a.offs[HSG_RES_DST(0) * B1 + d];
        const int64_t db = a.docbase[d], po = a.pairbase[d];
        for (int64_t i = threadIdx.x; i < cnt; i += kThreads) {
            const int64_t k = s0 + i;
            if (job == kPair) {
                const int64_t o = po + i;
                if (!inside(o, a.n_pair)) continue;
                a.pair_s[o] = (int64_t)a.c.pair_s[k] + so;
                a.pair_d[o] = (int64_t)a.c.pair_d[k] + db;
                a.doc_sent[o] = (int32_t)(a.c.doc_sent[k] + so);
                a.sent_doc[o] = (int32_t)(a.c.sent_doc[k] + db);
            } else if (job == kSent) {
                const int64_t o = so + i;
                if (!inside(o, a.n_sent)) continue;
                const int64_t ss = (int64_t)a.c.sent_super[k] + uo, ds = (int64_t)a.c.doc_super[k] + uo;
                a.sent_super64[o] = ss;
                a.doc_super64[o] = ds;
                a.sent_super[o] = (int32_t)ss;
                a.doc_super[o] = (int32_t)ds;
                a.sent_ptr[o] = (int32_t)(a.c.sent_ptr[k] + po);
                a.sent_row[o] = (int32_t)(a.c.sent_row[k] + uo);
                a.sup_list[o] = (int32_t)(a.c.sup_list[k] + so);
            } else if (job == kDocn) {
                const int64_t o = db + i;
                if (!inside(o, a.n_docn)) continue;
                a.inv_cnt[o] = a.c.inv_cnt[k];
                a.doc_ptr[o] = (int32_t)(a.c.doc_ptr[k] + po);
                a.doc_row[o] = (int32_t)(a.c.doc_row[k] + uo);
            } else {
                const int64_t o = uo + i;
                if (!inside(o, a.n_super)) continue;
                const int64_t code = a.c.sup_code[k], sent = a.c.sup_sent[k];
                a.super_pos[o] = code >= 0 ? so + code : a.n_sent + db + (-code - 1);
                a.super_src[o] = (int32_t)(code >= 0 ? so + code : code - db);
                a.sup_sent[o] = (int32_t)(sent >= 0 ? sent + so : -1);
                a.sup_ptr[o] = (int32_t)(a.c.sup_ptr[k] + so);
            }
        }
    }
}

}  // namespace

extern "C" int hsg_res_hdsg_supported(int B, int64_t n_sent, int64_t n_docn, int64_t n_pair, int64_t n_super) {
    return hsg_res_supported(B, n_sent, n_docn, n_pair) && n_super >= 0 && n_super <= kMaxCount;
}

extern "C" int hsg_res_hdsg(const hsg_res_store *st, const hsg_res_hdsg_cols *cols, int B, const int32_t *pick,
                            const int64_t *offs, const int32_t *docbase, const int32_t *pairbase, int64_t n_sent,
                            int64_t n_docn, int64_t n_pair, int64_t n_super, int64_t *pair_s, int64_t *pair_d,
                            int64_t *super_pos, int64_t *sent_super64, int64_t *doc_super64, float *inv_cnt,
                            int32_t *super_src, int32_t *doc_ptr, int32_t *doc_sent, int32_t *sent_ptr,
                            int32_t *sent_doc, int32_t *sent_row, int32_t *doc_row, int32_t *sent_super,
                            int32_t *doc_super, int32_t *sup_sent, int32_t *sup_ptr, int32_t *sup_list, void *stream) {
    if (!st || !pick || !st->starts || !st->bases || st->n_docs < 1 || st->n_docs > kMaxCount) return HSG_EINVAL;
    if (B < 1 || B > kMaxB || !cols || !offs || !docbase || !pairbase || !cols->dstart || !cols->pstart)
        return HSG_EINVAL;
    if (!hsg_res_hdsg_supported(B, n_sent, n_docn, n_pair, n_super) || !doc_ptr || !sent_ptr || !sup_ptr)
        return HSG_EINVAL;
    const hsg_res_hdsg_cols &c = *cols;
    if (n_pair > 0 && (!pair_s || !pair_d || !doc_sent || !sent_doc || !c.pair_s || !c.pair_d || !c.doc_sent ||
                       !c.sent_doc))
        return HSG_EINVAL;
    if (n_sent > 0 && (!sent_super64 || !doc_super64 || !sent_super || !doc_super || !sent_row || !sup_list ||
                       !c.sent_super || !c.doc_super || !c.sent_ptr || !c.sent_row || !c.sup_list))
        return HSG_EINVAL;
    if (n_docn > 0 && (!inv_cnt || !doc_row || !c.inv_cnt || !c.doc_ptr || !c.doc_row)) return HSG_EINVAL;
    if (n_super > 0 && (!super_pos || !super_src || !sup_sent || !c.sup_code || !c.sup_sent || !c.sup_ptr))
        return HSG_EINVAL;
    Args a{st->n_docs, st->starts, c,        B,        pick,     offs,     docbase,  pairbase,   n_sent,    n_docn,
           n_pair,     n_super,    pair_s,   pair_d,   super_pos, sent_super64, doc_super64, inv_cnt, super_src,
           doc_ptr,    doc_sent,   sent_ptr, sent_doc, sent_row, doc_row,  sent_super, doc_super, sup_sent, sup_ptr,
           sup_list};
    dim3 grid((unsigned)(B < kMaxBlocksX ? B : kMaxBlocksX), (unsigned)kJobs);
    k_res_hdsg<<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
