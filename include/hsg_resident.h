/*
 * hsg_resident.h -- C ABI of the device-resident document store (libhsg.so, gfx950): a batch
 * of documents is assembled on the device from a store that holds every document's graph
 * columns and both hot relations, by gathers with running offsets.  No sort, no host wait.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their own
 * (as include/hsg_train.h, hsg_model.h, hsg_embed.h and hsg_eval.h).  This header carries the
 * same two obligations itself: its declarations equal its entry in the binding's registry,
 * _lib.ABI["hsg_resident.h"] (tests/test_abi_conformance.py, which also holds the two structs
 * below to their ctypes mirrors), and every entry point below that writes through a pointer has
 * a guard-band case in tests/test_gpu_resident_guard.py.
 *
 * Conventions are hsg.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.  Integer
 * work only: the results are bitwise the same whatever the grid.  No block waits for another.
 */
#ifndef HSG_RESIDENT_H_
#define HSG_RESIDENT_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- count families ---------------------------------------------------------------------
 * Every stored column belongs to one family; a family says how many elements (rows) of the
 * column a document owns.  Per relation kind q (0 = W2S, 1 = S2W) there are three: the
 * relation's source nodes, its destination nodes and its typed edges. */
#define HSG_RES_NODE 0
#define HSG_RES_EDGE 1
#define HSG_RES_SENT 2
#define HSG_RES_SRC(q) (3 + 3 * (q))
#define HSG_RES_DST(q) (4 + 3 * (q))
#define HSG_RES_TYP(q) (5 + 3 * (q))
#define HSG_RES_NFAM 9

/* One relation of the store.  Every array is the concatenation over the documents, document
 * s owning the elements starts[f][s] .. starts[f][s+1]-1 of the array's family f:
 *   DST: indptr (WITHOUT a closing element), phantom, dst_nodes
 *   SRC: cindptr (without a closing element), src_nodes
 *   TYP: src, tf, eid, cdst, cperm
 * The values are those of hsg_rel_build on some batch that contained the document (a build
 * chunk); bases[f][s] is the count of family f that preceded the document in that batch. */
typedef struct hsg_res_rel {
    const int32_t *indptr, *src;
    const uint8_t *tf;
    const int32_t *eid, *phantom, *cindptr, *cdst, *cperm, *src_nodes, *dst_nodes;
} hsg_res_rel;

/* The store (a host struct of device pointers, read during the call only).
 *   starts int64 [HSG_RES_NFAM][n_docs + 1], non-decreasing per family;
 *   bases  int64 [HSG_RES_NFAM][n_docs].
 * Graph columns, narrowed:
 *   NODE: unit, ndtype uint8 (the float values 0..255); id int32; sent_rank int32: the row of
 *         the document's sentence columns that belongs to this node, or -1 (0 <= rank < the
 *         document's SENT count; anything else is treated as -1)
 *   SENT: words int32 [.][sent_len]; label uint8 [.][label_len]   (position is rank + 1)
 *   EDGE: src, dst int32, relative to the build chunk's first node (base: bases[NODE]);
 *         tffrac uint8; edtype uint8 (the float values 0..255)
 * A family with no element at all may have NULL columns. */
typedef struct hsg_res_store {
    int64_t n_docs;
    const int64_t *starts, *bases;
    int32_t sent_len, label_len;
    const uint8_t *unit, *ndtype;
    const int32_t *id, *sent_rank, *words;
    const uint8_t *label;
    const int32_t *src, *dst;
    const uint8_t *tffrac, *edtype;
    hsg_res_rel rel[2];
} hsg_res_store;

/* hsg_res_supported (host-only): 1 <= B <= 2^20 and 0 <= n_nodes, n_edges, n_typed <= 2^31-1
 * (the batch's totals; n_typed is the larger of the two kinds'). */
int hsg_res_supported(int B, int64_t n_nodes, int64_t n_edges, int64_t n_typed);

/* ---- running offsets ----------------------------------------------------------------------
 * pick int32 [B]: the store slots of the batch's documents in batch order; a slot may repeat.
 * A pick outside [0, n_docs) is an empty document in every family (nothing of the store is
 * read for it).
 *   offs int64 [HSG_RES_NFAM][B + 1]: offs[f][d] = sum over j < d of the count of family f of
 *   document pick[j]; offs[f][B] is the batch's total.  All 9 (B + 1) elements are written.
 * One launch of HSG_RES_NFAM blocks; a block scans its family in tiles, carrying the sum.
 * HSG_EINVAL: NULL st, pick, offs, st->starts or st->bases, n_docs < 1 or > 2^31-1, B outside
 * hsg_res_supported's range. */
int hsg_res_offsets(const hsg_res_store *st, int B, const int32_t *pick, int64_t *offs, void *stream);

/* ---- graph columns --------------------------------------------------------------------------
 * offs as written by hsg_res_offsets for the same (st, B, pick); n_nodes = offs[NODE][B] and
 * n_edges = offs[EDGE][B] as the caller knows them (they size the outputs: an element whose
 * index is not below them is not written, whatever offs holds).
 * With d the document, s = pick[d], i a node / j an edge of the document, N0 = offs[NODE][d]:
 *   unit, ndtype float [n_nodes]:  the stored bytes as floats
 *   id int64 [n_nodes]
 *   words int64 [n_nodes][sent_len], label int64 [n_nodes][label_len], position int64
 *     [n_nodes][1]: the sentence row sent_rank (position: rank + 1) on nodes that have one,
 *     zero rows elsewhere
 *   src, dst int64 [n_edges]: stored value - bases[NODE][s] + N0
 *   tffrac int64 [n_edges]; edtype float [n_edges]
 * Every element is written exactly once; nothing else is.  One launch.
 * HSG_EINVAL: as hsg_res_offsets, NULL offs, sent_len < 1, label_len < 1, sizes that
 * hsg_res_supported declines, a NULL node output with n_nodes > 0 or edge output with
 * n_edges > 0. */
int hsg_res_graph(const hsg_res_store *st, int B, const int32_t *pick, const int64_t *offs, int64_t n_nodes,
                  int64_t n_edges, float *unit, float *ndtype, int64_t *id, int64_t *words, int64_t *position,
                  int64_t *label, int64_t *src, int64_t *dst, int64_t *tffrac, float *edtype, void *stream);

/* ---- one relation, in struct hsg_rel's layout (include/hsg.h) -----------------------------
 * kind 0 = W2S, 1 = S2W.  n_src, n_dst, n_typed: offs[SRC(kind)][B], offs[DST(kind)][B],
 * offs[TYP(kind)][B] as the caller knows them (they size the outputs, as above).  Each output
 * is the concatenation over the picked documents of the stored slice plus
 * (offs[g][d] - bases[g][s]) for the family g named here:
 *   indptr  int32 [n_dst + 1]   + TYP; indptr[n_dst] = n_typed of offs (the closing element)
 *   src     int32 [n_typed]     + SRC
 *   tf      uint8 [n_typed]
 *   eid     int64 [n_typed]     + EDGE
 *   phantom int32 [n_dst]
 *   cindptr int32 [n_src + 1]   + TYP; cindptr[n_src] = n_typed of offs
 *   cdst    int32 [n_typed]     + DST
 *   cperm   int32 [n_typed]     + TYP
 *   src_nodes int64 [n_src], dst_nodes int64 [n_dst]   + NODE
 * Every element is written exactly once; nothing else is.  One launch.
 * HSG_EINVAL: as hsg_res_graph, kind outside {0, 1}, NULL indptr or cindptr, a NULL output
 * whose extent is not empty. */
int hsg_res_relation(const hsg_res_store *st, int kind, int B, const int32_t *pick, const int64_t *offs,
                     int64_t n_src, int64_t n_dst, int64_t n_typed, int32_t *indptr, int32_t *src, uint8_t *tf,
                     int64_t *eid, int32_t *phantom, int32_t *cindptr, int32_t *cdst, int32_t *cperm,
                     int64_t *src_nodes, int64_t *dst_nodes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_RESIDENT_H_ */
