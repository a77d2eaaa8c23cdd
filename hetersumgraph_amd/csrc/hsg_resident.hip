// hsg_resident.hip -- batch assembly from the device-resident document store for gfx950.
// C ABI and the whole contract: include/hsg_resident.h.
//
// A document's graph columns and its two hot relations do not depend on the batch it lands
// in, except through five running offsets (node, edge, source rank, destination rank, typed
// edge).  The store keeps them once; a batch is three kinds of launch:
//
//   k_res_offsets   one block per count family: the exclusive prefix sums of the picked
//                   documents' counts, scanned in tiles of kScan with a carried sum.
//   k_res_gather    every column of one entry point in ONE launch: blockIdx.y is the column
//                   (a table in the kernel arguments), blockIdx.x walks (document, part)
//                   units, a part being the p-th of kParts near-equal runs of the document's
//                   elements.  An element is read once, widened, offset and written once.
//
// Pure integer copies: nothing is accumulated, so the result cannot depend on the grid.  The
// traffic is the outputs' bytes (the store's columns are 2 to 8 times narrower); the int64
// sentence columns dominate (n_nodes x (sent_len + label_len + 1) x 8 bytes, mostly zero rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_resident.h"

namespace {

constexpr int kScan = 256;          // threads of an offsets block (= its scan tile)
constexpr int kThreads = 256;       // threads of a gather block
constexpr int kWave = 64;
constexpr int kParts = 8;           // runs per document (fewer once B alone fills the device)
constexpr int kMaxBlocksX = 4096;
constexpr int kMaxCols = 10;
constexpr int kMaxB = 1 << 20;
constexpr int64_t kMaxCount = 2147483647LL;

enum ColKind : int {
    kU8F32 = 0,     // uint8 -> float
    kU8I64,         // uint8 -> int64
    kU8U8,          // uint8 -> uint8
    kI32I64,        // int32 + add -> int64
    kI32I32,        // int32 + add -> int32
    kRowsI32,       // sentence rows int32 [.][width] -> int64 rows on the nodes
    kRowsU8,        // sentence rows uint8 [.][width] -> int64 rows on the nodes
    kPosition,      // sent_rank + 1 (0 where there is no sentence row) -> int64
};

struct Col {
    const void *in;
    void *out;
    int kind;
    int fam;        // family of the output's elements (and of `in`, except the row kinds: SENT)
    int add;        // family whose (new base - stored base) is added, or -1
    int width;      // row kinds
    int closing;    // also write out[offs[fam][B]] = offs[add][B]
    int64_t limit;  // elements (rows) of `out`: nothing at or past it is written
};

struct Cols {
    Col c[kMaxCols];
};

struct View {
    int64_t n_docs;
    const int64_t *starts, *bases;
    const int32_t *sent_rank;
    int B;
    const int32_t *pick;
};

__global__ __launch_bounds__(kScan) void k_res_offsets(View v, int64_t *__restrict__ offs) {
    __shared__ int64_t s_scan[kScan];
    const int f = blockIdx.x, t = threadIdx.x;
    const int64_t *st = v.starts + (int64_t)f * (v.n_docs + 1);
    int64_t *o = offs + (int64_t)f * (v.B + 1);
    int64_t carry = 0;
    if (t == 0) o[0] = 0;
    for (int d0 = 0; d0 < v.B; d0 += kScan) {
        const int d = d0 + t;
        int64_t c = 0;
        if (d < v.B) {
            const uint32_t s = (uint32_t)v.pick[d];
            if ((int64_t)s < v.n_docs) c = st[s + 1] - st[s];
        }
        s_scan[t] = c;
        __syncthreads();
        for (int k = 1; k < kScan; k <<= 1) {              // inclusive Hillis-Steele scan of the tile
            const int64_t x = t >= k ? s_scan[t - k] : 0;
            __syncthreads();
            s_scan[t] += x;
            __syncthreads();
        }
        if (d < v.B) o[d + 1] = carry + s_scan[t];
        carry += s_scan[kScan - 1];
        __syncthreads();
    }
}

template <typename S, typename D>
__device__ inline void copy_run(const S *__restrict__ in, D *__restrict__ out, int64_t lo, int64_t hi, int64_t s0,
                                int64_t o0, int64_t add, int64_t limit) {
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
        const int64_t o = o0 + i;
        if (o < limit) out[o] = (D)((int64_t)in[s0 + i] + add);
    }
}

template <typename S>
__device__ inline void rows_run(const S *__restrict__ in, int64_t *__restrict__ out, const int32_t *__restrict__ rank,
                                int64_t lo, int64_t hi, int64_t n0, int64_t o0, int64_t r0, int64_t rows, int width,
                                int64_t limit) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int64_t i = lo + wave; i < hi; i += kThreads / kWave) {
        const int64_t o = o0 + i;
        if (o >= limit) continue;
        const uint32_t r = (uint32_t)rank[n0 + i];
        const bool has = (int64_t)r < rows;
        const S *src = in + (r0 + (has ? (int64_t)r : 0)) * width;
        int64_t *dst = out + o * width;
        for (int c = lane; c < width; c += kWave) dst[c] = has ? (int64_t)src[c] : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_res_gather(View v, Cols cols, const int64_t *__restrict__ offs,
                                                          int parts) {
    const Col &c = cols.c[blockIdx.y];
    const int64_t B1 = (int64_t)v.B + 1;
    const int64_t *st = v.starts + (int64_t)c.fam * (v.n_docs + 1);
    const int64_t units = (int64_t)v.B * parts;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int d = (int)(u / parts), p = (int)(u % parts);
        const uint32_t s = (uint32_t)v.pick[d];
        if ((int64_t)s >= v.n_docs) continue;
        const int64_t s0 = st[s], cnt = st[s + 1] - s0;
        const int64_t lo = cnt / parts * p + min((int64_t)p, cnt % parts);
        const int64_t hi = lo + cnt / parts + (p < cnt % parts ? 1 : 0);
        if (lo >= hi) continue;
        const int64_t o0 = offs[c.fam * B1 + d];
        const int64_t add = c.add >= 0 ? offs[c.add * B1 + d] - v.bases[(int64_t)c.add * v.n_docs + s] : 0;
        switch (c.kind) {
        case kU8F32:
            copy_run((const uint8_t *)c.in, (float *)c.out, lo, hi, s0, o0, 0, c.limit);
            break;
        case kU8I64:
            copy_run((const uint8_t *)c.in, (int64_t *)c.out, lo, hi, s0, o0, 0, c.limit);
            break;
        case kU8U8:
            copy_run((const uint8_t *)c.in, (uint8_t *)c.out, lo, hi, s0, o0, 0, c.limit);
            break;
        case kI32I64:
            copy_run((const int32_t *)c.in, (int64_t *)c.out, lo, hi, s0, o0, add, c.limit);
            break;
        case kI32I32:
            copy_run((const int32_t *)c.in, (int32_t *)c.out, lo, hi, s0, o0, add, c.limit);
            break;
        default: {
            // row kinds: the output's elements are the document's nodes, the input's its sentence rows
            const int64_t *ss = v.starts + (int64_t)HSG_RES_SENT * (v.n_docs + 1);
            const int64_t r0 = ss[s], rows = ss[s + 1] - r0;
            if (c.kind == kRowsI32) {
                rows_run((const int32_t *)c.in, (int64_t *)c.out, v.sent_rank, lo, hi, s0, o0, r0, rows, c.width, c.limit);
            } else if (c.kind == kRowsU8) {
                rows_run((const uint8_t *)c.in, (int64_t *)c.out, v.sent_rank, lo, hi, s0, o0, r0, rows, c.width, c.limit);
            } else {
                int64_t *out = (int64_t *)c.out;
                for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
                    const uint32_t r = (uint32_t)v.sent_rank[s0 + i];
                    if (o0 + i < c.limit) out[o0 + i] = (int64_t)r < rows ? (int64_t)r + 1 : 0;
                }
            }
        }
        }
    }
    if (c.closing && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t at = offs[c.fam * B1 + v.B];
        if (at < c.limit) ((int32_t *)c.out)[at] = (int32_t)offs[c.add * B1 + v.B];
    }
}

bool view_of(const hsg_res_store *st, int B, const int32_t *pick, View *v) {
    if (!st || !pick || !st->starts || !st->bases || st->n_docs < 1 || st->n_docs > kMaxCount) return false;
    if (B < 1 || B > kMaxB) return false;
    *v = View{st->n_docs, st->starts, st->bases, st->sent_rank, B, pick};
    return true;
}

int gather(const View &v, const Cols &cols, int ncol, const int64_t *offs, hipStream_t s) {
    const int parts = v.B >= kMaxBlocksX / kParts ? 1 : kParts;
    const int64_t units = (int64_t)v.B * parts;
    dim3 grid((unsigned)(units < kMaxBlocksX ? units : kMaxBlocksX), (unsigned)ncol);
    k_res_gather<<<grid, kThreads, 0, s>>>(v, cols, offs, parts);
    return (int)hipGetLastError();
}

Col col(const void *in, void *out, int kind, int fam, int add, int64_t limit, int width = 1, int closing = 0) {
    return Col{in, out, kind, fam, add, width, closing, limit};
}

}  // namespace

extern "C" int hsg_res_supported(int B, int64_t n_nodes, int64_t n_edges, int64_t n_typed) {
    return B >= 1 && B <= kMaxB && n_nodes >= 0 && n_nodes <= kMaxCount && n_edges >= 0 && n_edges <= kMaxCount &&
           n_typed >= 0 && n_typed <= kMaxCount;
}

extern "C" int hsg_res_offsets(const hsg_res_store *st, int B, const int32_t *pick, int64_t *offs, void *stream) {
    View v;
    if (!view_of(st, B, pick, &v) || !offs) return HSG_EINVAL;
    k_res_offsets<<<HSG_RES_NFAM, kScan, 0, (hipStream_t)stream>>>(v, offs);
    return (int)hipGetLastError();
}

extern "C" int hsg_res_graph(const hsg_res_store *st, int B, const int32_t *pick, const int64_t *offs,
                             int64_t n_nodes, int64_t n_edges, float *unit, float *ndtype, int64_t *id,
                             int64_t *words, int64_t *position, int64_t *label, int64_t *src, int64_t *dst,
                             int64_t *tffrac, float *edtype, void *stream) {
    View v;
    if (!view_of(st, B, pick, &v) || !offs || st->sent_len < 1 || st->label_len < 1) return HSG_EINVAL;
    if (!hsg_res_supported(B, n_nodes, n_edges, 0)) return HSG_EINVAL;
    if (n_nodes > 0 && (!unit || !ndtype || !id || !words || !position || !label)) return HSG_EINVAL;
    if (n_edges > 0 && (!src || !dst || !tffrac || !edtype)) return HSG_EINVAL;
    const int N = HSG_RES_NODE, E = HSG_RES_EDGE;
    Cols c;
    c.c[0] = col(st->words, words, kRowsI32, N, -1, n_nodes, st->sent_len);
    c.c[1] = col(st->label, label, kRowsU8, N, -1, n_nodes, st->label_len);
    c.c[2] = col(nullptr, position, kPosition, N, -1, n_nodes);
    c.c[3] = col(st->unit, unit, kU8F32, N, -1, n_nodes);
    c.c[4] = col(st->ndtype, ndtype, kU8F32, N, -1, n_nodes);
    c.c[5] = col(st->id, id, kI32I64, N, -1, n_nodes);
    c.c[6] = col(st->src, src, kI32I64, E, N, n_edges);
    c.c[7] = col(st->dst, dst, kI32I64, E, N, n_edges);
    c.c[8] = col(st->tffrac, tffrac, kU8I64, E, -1, n_edges);
    c.c[9] = col(st->edtype, edtype, kU8F32, E, -1, n_edges);
    return gather(v, c, 10, offs, (hipStream_t)stream);
}

extern "C" int hsg_res_relation(const hsg_res_store *st, int kind, int B, const int32_t *pick, const int64_t *offs,
                                int64_t n_src, int64_t n_dst, int64_t n_typed, int32_t *indptr, int32_t *src,
                                uint8_t *tf, int64_t *eid, int32_t *phantom, int32_t *cindptr, int32_t *cdst,
                                int32_t *cperm, int64_t *src_nodes, int64_t *dst_nodes, void *stream) {
    View v;
    if (!view_of(st, B, pick, &v) || !offs || (kind != 0 && kind != 1) || !indptr || !cindptr) return HSG_EINVAL;
    if (!hsg_res_supported(B, n_src, n_dst, n_typed)) return HSG_EINVAL;
    if (n_typed > 0 && (!src || !tf || !eid || !cdst || !cperm)) return HSG_EINVAL;
    if ((n_dst > 0 && (!phantom || !dst_nodes)) || (n_src > 0 && !src_nodes)) return HSG_EINVAL;
    const int S = HSG_RES_SRC(kind), D = HSG_RES_DST(kind), T = HSG_RES_TYP(kind);
    const hsg_res_rel &r = st->rel[kind];
    Cols c;
    c.c[0] = col(r.eid, eid, kI32I64, T, HSG_RES_EDGE, n_typed);
    c.c[1] = col(r.src, src, kI32I32, T, S, n_typed);
    c.c[2] = col(r.cdst, cdst, kI32I32, T, D, n_typed);
    c.c[3] = col(r.cperm, cperm, kI32I32, T, T, n_typed);
    c.c[4] = col(r.tf, tf, kU8U8, T, -1, n_typed);
    c.c[5] = col(r.indptr, indptr, kI32I32, D, T, n_dst + 1, 1, 1);
    c.c[6] = col(r.phantom, phantom, kI32I32, D, -1, n_dst);
    c.c[7] = col(r.dst_nodes, dst_nodes, kI32I64, D, HSG_RES_NODE, n_dst);
    c.c[8] = col(r.cindptr, cindptr, kI32I32, S, T, n_src + 1, 1, 1);
    c.c[9] = col(r.src_nodes, src_nodes, kI32I64, S, HSG_RES_NODE, n_src);
    return gather(v, c, 10, offs, (hipStream_t)stream);
}
