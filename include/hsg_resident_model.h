/*
 * hsg_resident_model.h -- C ABI of the model view of a resident batch (libhsg.so, gfx950): the
 * index structures the model builds first thing from a batch -- the sentence node list, the
 * sentences' token rows and CNN row layout, the LSTM's document layout and the tf-idf table
 * index -- assembled on the device from the resident store, beside include/hsg_resident.h's
 * batch.  They are pure functions of the picked documents and the running offsets.
 *
 * These entry points live in the same libhsg.so, in a header of their own: its declarations
 * equal its entry in the binding's registry, _lib.ABI["hsg_resident_model.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a pointer
 * has a guard-band case in tests/test_gpu_resident_model_guard.py.
 *
 * Conventions are hsg_resident.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.  Integer
 * work only: the results are bitwise the same whatever the grid.  No block waits for another.
 */
#ifndef HSG_RESIDENT_MODEL_H_
#define HSG_RESIDENT_MODEL_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_res_model_supported (host-only): hsg_res_supported(B, n_sent, n_edges, 0) and
 * 0 <= n_rows <= 2^31-1 (rowoff is int32). */
int hsg_res_model_supported(int B, int64_t n_sent, int64_t n_edges, int64_t n_rows);

/* ---- the model view of a batch ---------------------------------------------------------------
 * Two more columns of the store's SENT family (document s owns the elements
 * starts[SENT][s] .. starts[SENT][s+1]-1, as st->words' rows):
 *   tok_len int32: the sentence's length, the number of its non-zero tokens
 *   tok_row int32: the exclusive prefix sum of (tok_len + 1) inside the document
 * The store's build has checked that every non-zero token precedes the first zero and that the
 * document's sentence nodes are exactly its ndtype == 1 nodes, ascending in node id with
 * their sent_rank; the outputs below equal the model's own constructions only then.
 *
 * st, B, pick, offs: as hsg_res_graph's.  rowbase int32 [B + 1]: rowbase[d] = the sum over
 * j < d of the CNN row count (sum of tok_len + 1) of document pick[j], 0 for a pick outside
 * [0, n_docs) -- the caller sums it from the row counts it keeps per document.  n_sent =
 * offs[SENT][B], n_edges = offs[EDGE][B] as the caller knows them (they size the outputs: an
 * element whose index is not below them is not written, whatever offs and rowbase hold).
 *
 * With d the document, s = pick[d], r a sentence row of it (0 <= r < its SENT count),
 * g = offs[SENT][d] + r, i the node of the document with sent_rank[i] == r:
 *   sent_nodes  int64 [n_sent]           offs[NODE][d] + i
 *   sent_ids    int64 [n_sent][sent_len] the stored token row, widened
 *   sent_pos    int64 [n_sent]           r + 1
 *   sent_len    int64 [n_sent]           tok_len
 *   rowoff      int32 [n_sent + 1]       rowbase[d] + tok_row; rowoff[n_sent] = rowbase[B]
 *   doc_off     int32 [B + 1]            offs[SENT][0..B], narrowed
 *   prev        int64 [n_sent][2]        [0]: g - 1, or n_sent for r == 0;
 *                                        [1]: g + 1, or n_sent for the document's last row
 *   tfidf_index int64 [n_edges]          edtype == 0 ? tffrac : -1, in the batch's edge order
 * A pick outside [0, n_docs) is an empty document.  Every element is written exactly once
 * (sent_nodes: given the store's check that the ranks 0 .. count-1 occur once each); nothing
 * else is.  One launch.
 * HSG_EINVAL: as hsg_res_offsets, NULL offs or rowbase, sent_len < 1, sizes that
 * hsg_res_model_supported declines, NULL rowoff or doc_off, a NULL sentence output or store
 * column with n_sent > 0, NULL tfidf_index with n_edges > 0. */
int hsg_res_model(const hsg_res_store *st, const int32_t *tok_len, const int32_t *tok_row, int B,
                  const int32_t *pick, const int64_t *offs, const int32_t *rowbase, int64_t n_sent,
                  int64_t n_edges, int64_t *sent_nodes, int64_t *sent_ids, int64_t *sent_pos, int64_t *sent_len,
                  int32_t *rowoff, int32_t *doc_off, int64_t *prev, int64_t *tfidf_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_RESIDENT_MODEL_H_ */
