/*
 * hsg_resident_hdsg.h -- C ABI of the doc view of a resident batch (libhsg.so, gfx950): the
 * doc-side index structures HSumDocGraph builds on the host from a multi-document batch -- the
 * sentence -> doc pair list, the supernode order and the per-sentence supernode rows
 * (HiGraph._hdsg_layout), and the CSR / CSC forms of the pair list with the inverse supernode
 * lists the native glue walks (head.HeadLayout) -- assembled on the device from the resident
 * store, beside include/hsg_resident_model.h's model view.  Every one of them is, per document,
 * a stored local value plus a running offset of its family.
 *
 * These entry points live in the same libhsg.so, in a header of their own: its declarations
 * equal its entry in the binding's registry, _lib.ABI["hsg_resident_hdsg.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a pointer
 * has a guard-band case in tests/test_gpu_resident_hdsg_guard.py.
 *
 * Conventions are hsg_resident.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.  Integer
 * work and copies only (inv_cnt is copied, never computed): the results are bitwise the same
 * whatever the grid.  No block waits for another.
 */
#ifndef HSG_RESIDENT_HDSG_H_
#define HSG_RESIDENT_HDSG_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The store's doc-view columns (a host struct of device pointers, beside hsg_res_store).  Four
 * element families per document s:
 *   SENT  its sentences:              starts[HSG_RES_SENT][s]    .. (hsg_res_store)
 *   SUP   its supernodes (unit == 1): starts[HSG_RES_DST(0)][s]  .. (hsg_res_store)
 *   DOCN  its doc nodes (ndtype == 2): dstart[s] .. dstart[s+1]-1
 *   PAIR  its sentence -> doc edges:   pstart[s] .. pstart[s+1]-1
 * Every value is local to the document: what the host constructions give for the document as
 * a batch of one.  The store's build has checked that every document has a doc node, a pair
 * for every doc node, a doc for every sentence, and that its supernodes are exactly its
 * sentence and doc nodes; the outputs below equal the host's only then. */
typedef struct hsg_res_hdsg_cols {
    const int64_t *dstart;      /* [n_docs + 1] exclusive prefix sums of the DOCN counts            */
    const int64_t *pstart;      /* [n_docs + 1] exclusive prefix sums of the PAIR counts            */
    const int32_t *pair_s;      /* PAIR  sentence rank of the pair, in edge order                    */
    const int32_t *pair_d;      /* PAIR  doc rank of the pair, in edge order                         */
    const int32_t *doc_sent;    /* PAIR  sentence ranks by ascending doc rank, ties in edge order    */
    const int32_t *sent_doc;    /* PAIR  doc ranks by ascending sentence rank, ties in edge order    */
    const int32_t *sent_super;  /* SENT  supernode rank of the sentence                              */
    const int32_t *doc_super;   /* SENT  supernode rank of the sentence's doc (its last pair's)      */
    const int32_t *sent_ptr;    /* SENT  first position of the sentence in sent_doc                  */
    const int32_t *sent_row;    /* SENT  supernode row that holds the sentence                       */
    const int32_t *sup_list;    /* SENT  sentence ranks by ascending doc_super, ties ascending       */
    const float *inv_cnt;       /* DOCN  1 / max(pairs of the doc node, 1), as the host rounds it    */
    const int32_t *doc_ptr;     /* DOCN  first position of the doc node in doc_sent                  */
    const int32_t *doc_row;     /* DOCN  supernode row that holds the doc node                       */
    const int32_t *sup_code;    /* SUP   sentence rank r as r, doc rank k as -(k + 1)                */
    const int32_t *sup_sent;    /* SUP   sentence rank of a sentence supernode, -1 for a doc's       */
    const int32_t *sup_ptr;     /* SUP   first position of the supernode in sup_list                 */
} hsg_res_hdsg_cols;

/* hsg_res_hdsg_supported (host-only): 1 <= B <= 2^20 and every count in [0, 2^31-1]. */
int hsg_res_hdsg_supported(int B, int64_t n_sent, int64_t n_docn, int64_t n_pair, int64_t n_super);

/* ---- the doc view of a batch -------------------------------------------------------------------
 * st, B, pick, offs: as hsg_res_graph's.  docbase, pairbase int32 [B + 1]: the sums over j < d
 * of the DOCN / PAIR counts of document pick[j], 0 for a pick outside [0, n_docs) -- the caller
 * sums them from the counts it keeps per document.  n_sent = offs[SENT][B], n_super =
 * offs[DST(0)][B], n_docn = docbase[B], n_pair = pairbase[B] as the caller knows them (they size
 * the outputs: an element whose index is not in [0, its count) is not written, whatever offs,
 * docbase and pairbase hold).
 *
 * With d the document, s = pick[d], so = offs[SENT][d], uo = offs[DST(0)][d], do = docbase[d],
 * po = pairbase[d] and c the stored local value of the element:
 *   pair_s      int64 [n_pair]      po + i:  c.pair_s + so
 *   pair_d      int64 [n_pair]      po + i:  c.pair_d + do
 *   super_pos   int64 [n_super]     uo + i:  c.sup_code >= 0 ? so + c : n_sent + do + (-c - 1)
 *   sent_super64, doc_super64 int64 [n_sent]   so + i:  c.sent_super + uo, c.doc_super + uo
 *   inv_cnt     float [n_docn]      do + i:  c.inv_cnt, copied
 *   super_src   int32 [n_super]     uo + i:  c.sup_code >= 0 ? so + c : c - do
 *   doc_ptr     int32 [n_docn + 1]  do + i:  c.doc_ptr + po;   doc_ptr[n_docn] = n_pair
 *   doc_sent    int32 [n_pair]      po + i:  c.doc_sent + so
 *   sent_ptr    int32 [n_sent + 1]  so + i:  c.sent_ptr + po;  sent_ptr[n_sent] = n_pair
 *   sent_doc    int32 [n_pair]      po + i:  c.sent_doc + do
 *   sent_row    int32 [n_sent]      so + i:  c.sent_row + uo
 *   doc_row     int32 [n_docn]      do + i:  c.doc_row + uo
 *   sent_super, doc_super int32 [n_sent]       the int64 outputs' values, narrowed
 *   sup_sent    int32 [n_super]     uo + i:  c.sup_sent >= 0 ? c + so : -1
 *   sup_ptr     int32 [n_super + 1] uo + i:  c.sup_ptr + so;   sup_ptr[n_super] = n_sent
 *   sup_list    int32 [n_sent]      so + i:  c.sup_list + so
 * A pick outside [0, n_docs) is an empty document.  Every element is written exactly once;
 * nothing else is.  One launch.
 * HSG_EINVAL: as hsg_res_offsets, NULL cols, offs, docbase or pairbase, NULL cols->dstart or
 * cols->pstart, sizes that hsg_res_hdsg_supported declines, NULL doc_ptr, sent_ptr or sup_ptr,
 * and per family with a positive count a NULL output or stored column of it. */
int hsg_res_hdsg(const hsg_res_store *st, const hsg_res_hdsg_cols *cols, int B, const int32_t *pick,
                 const int64_t *offs, const int32_t *docbase, const int32_t *pairbase, int64_t n_sent,
                 int64_t n_docn, int64_t n_pair, int64_t n_super, int64_t *pair_s, int64_t *pair_d,
                 int64_t *super_pos, int64_t *sent_super64, int64_t *doc_super64, float *inv_cnt,
                 int32_t *super_src, int32_t *doc_ptr, int32_t *doc_sent, int32_t *sent_ptr, int32_t *sent_doc,
                 int32_t *sent_row, int32_t *doc_row, int32_t *sent_super, int32_t *doc_super, int32_t *sup_sent,
                 int32_t *sup_ptr, int32_t *sup_list, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_RESIDENT_HDSG_H_ */
