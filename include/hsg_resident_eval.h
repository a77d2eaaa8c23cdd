/*
 * hsg_resident_eval.h -- C ABI of the eval view of a resident batch (libhsg.so, gfx950): the
 * blocking operand of the native evaluation step on word ids (include/hsg_eval_words.h), one
 * int32 buffer [word_ptr (n_sent + 1) | word_ids (n_words, at least one element)] -- what
 * evalsel.pack_words joins on the host from the documents' (ptr, ids) pairs -- assembled on the
 * device from the resident store, beside include/hsg_resident_model.h's model view and
 * include/hsg_resident_hdsg.h's doc view and independent of both.  Per document it is a stored
 * local value plus the running word offset (the row ends), or a stored value copied (the ids).
 *
 * These entry points live in the same libhsg.so, in a header of their own: its declarations
 * equal its entry in the binding's registry, _lib.ABI["hsg_resident_eval.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a pointer
 * has a guard-band case in tests/test_gpu_resident_eval_guard.py.
 *
 * Conventions are hsg_resident.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.  Integer
 * work and copies only: the results are bitwise the same whatever the grid.  No block waits
 * for another.
 */
#ifndef HSG_RESIDENT_EVAL_H_
#define HSG_RESIDENT_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The store's eval-view columns (a host struct of device pointers, beside hsg_res_store).  Two
 * element families per document s:
 *   SENT  its sentence rows: starts[HSG_RES_SENT][s] ..            (hsg_res_store)
 *   WORD  its words:         wstart[s] .. wstart[s+1]-1, W_s = wstart[s+1] - wstart[s] of them
 * Every value is local to the document: evalsel.word_ids' (ptr, ids) of the document's own rows.
 * The store's build has checked ptr[0] == 0, ptr non-decreasing and ptr[rows] == W_s; the kernel
 * clamps a row end into [0, W_s] all the same, so no output points outside the batch's words.
 * A family with no element at all may have a NULL column. */
typedef struct hsg_res_eval_cols {
    const int64_t *wstart;      /* [n_docs + 1] exclusive prefix sums of the WORD counts            */
    const int32_t *wend;        /* SENT  ptr[i + 1] of the document's pair: where row i's words end  */
    const int32_t *wid;         /* WORD  the document-local word ids, as given                       */
} hsg_res_eval_cols;

/* hsg_res_eval_supported (host-only): 1 <= B <= 2^20, n_sent >= 0, n_words >= 0 and the pack's
 * n_sent + 1 + max(n_words, 1) elements at most 2^31-1. */
int hsg_res_eval_supported(int B, int64_t n_sent, int64_t n_words);

/* ---- the eval view of a batch ------------------------------------------------------------------
 * st, B, pick, offs: as hsg_res_graph's.  wordbase int32 [B + 1]: the sums over j < d of the WORD
 * counts of document pick[j], 0 for a pick outside [0, n_docs) -- the caller sums them from the
 * counts it keeps per document.  n_sent = offs[SENT][B] and n_words = wordbase[B] as the caller
 * knows them (they size the output: an element whose index is not in [0, its count) is not
 * written, whatever offs and wordbase hold).
 *
 *   pack int32 [n_sent + 1 + max(n_words, 1)]
 * With d the document, s = pick[d], so = offs[SENT][d], wo = wordbase[d]:
 *   pack[0]                   = 0
 *   pack[1 + so + i]          = wo + clamp(wend[starts[SENT][s] + i], 0, W_s)    i < the SENT count
 *   pack[n_sent + 1 + wo + k] = wid[wstart[s] + k]                               k < W_s
 *   pack[n_sent + 1]          = 0 when n_words == 0 (the one padding element)
 * A pick outside [0, n_docs) is an empty document.  Every element is written exactly once;
 * nothing else is.  One launch over the n_sent + n_words elements; each finds its document by a
 * search over the B + 1 offsets of its family.
 * HSG_EINVAL: as hsg_res_offsets, NULL cols, offs, wordbase, pack or cols->wstart, sizes that
 * hsg_res_eval_supported declines, a NULL cols->wend with n_sent > 0 or cols->wid with
 * n_words > 0. */
int hsg_res_eval(const hsg_res_store *st, const hsg_res_eval_cols *cols, int B, const int32_t *pick,
                 const int64_t *offs, const int32_t *wordbase, int64_t n_sent, int64_t n_words, int32_t *pack,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_RESIDENT_EVAL_H_ */
