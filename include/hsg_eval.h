/*
 * hsg_eval.h -- C ABI of the evaluation step's sentence selection (libhsg.so, gfx950): per
 * document, the top-m selection of Tester.py:105-140 with or without n-gram blocking
 * (Tester.py:155-184), the m == 0 rule (Tester.py:120-122) and the four match counters
 * (Tester.py:133-137), in ONE launch per batch and without a host round trip.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their
 * own (as include/hsg_train.h, hsg_model.h and hsg_embed.h).  This header carries the same
 * two obligations itself: its declarations equal its entry in the binding's registry,
 * _lib.ABI["hsg_eval.h"] (tests/test_abi_conformance.py),
 * and every entry point below that writes through a pointer has a guard-band case in
 * tests/test_gpu_eval_guard.py.
 *
 * Conventions are hsg.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.
 */
#ifndef HSG_EVAL_H_
#define HSG_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_eval_select_supported (host-only): 1 <= n_max <= 1024 and 0 <= gram_max <= 262144 (a
 * 32 KB bitmap in LDS, beside the scores, the order and the selection flags). */
int hsg_eval_select_supported(int n_max, int gram_max);

/* ---- selection, one wavefront per document ------------------------------------------------
 * Inputs.
 *   logits [n][2] fp32 contiguous; labels int64 [n], the class of each row.
 *   doc_off int32 [B+1]: document d owns rows doc_off[d] .. doc_off[d+1]-1, N_d of them
 *     (offsets are clamped to [0, n], as in hsg_doc_ce); "local index" means row - doc_off[d].
 *   m >= 0: sentences to choose per document (0: the argmax rule below).
 *   n_max: the largest document the caller admits (sizes the LDS arrays).
 *   gram_ptr int32 [n+1] or NULL (no blocking): the n-gram ids of row i are
 *     gram_ids[gram_ptr[i] .. gram_ptr[i+1]).  gram_ids holds gram_ptr[n] entries; every
 *     gram_ptr value is clamped to [0, gram_ptr[n]] and an end below its start is an empty
 *     list, so nothing outside gram_ids is read whatever gram_ptr holds.  Ids are
 *     document-local and dense: 0 <= id < gram_cnt[d], gram_cnt int32 [B].  gram_max: the
 *     largest gram_cnt[d] the caller admits (sizes the bitmap).
 *
 * Candidate order (m > 0).  Candidates are ordered by logits[i][1] descending AS FLOATS:
 * -0.0 == 0.0; NaN is greater than every number (where torch puts it) and all NaNs are
 * equal; equal keys are ordered by ascending local index.  This is a total order.  It is
 * this project's rule, not the reference's, whose order among equal scores is whatever
 * torch.sort / torch.topk happen to return.
 *
 * Selection without blocking (m > 0, gram_ptr == NULL): the first k = min(m, N_d) candidates
 * of that order.
 *
 * Selection with blocking (m > 0, gram_ptr != NULL), Tester.py:155-184: walk the candidates
 * in order; skip a candidate if any of its ids is already in the document's seen set;
 * otherwise choose it and add all its ids to the seen set; stop once k are chosen or the
 * candidates run out (fewer than k may survive).  Ids of a skipped sentence are not added.
 * A sentence's own repeated ids do not block it (test first, then set).  A sentence without
 * ids is never blocked.
 *
 * Selection for m == 0 (Tester.py:120-122): row i is selected iff argmax(logits[i]) != 0
 * with torch's NaN rule, i.e. iff !isnan(p0) && (isnan(p1) || p1 > p0); selected rows are
 * written in ascending index order.  Blocking is ignored, as in the reference: gram_ptr,
 * gram_ids and gram_cnt are not read and only the n_max refusal below applies.
 *
 * Outputs.
 *   sel int32 [B][sel_ld]: sel[d][0 .. nsel[d]) are the chosen local indices in choice order,
 *     the rest of the row up to sel_ld is -1.  sel_ld >= min(m, n_max), or >= n_max for m == 0.
 *   nsel int32 [B].
 *   doc_counts int32 [B][4] = { pred, true, match_true, match } of Tester.py:133-137 with
 *     prediction_i = 1 iff row i is selected: pred = nsel[d], true = the integer sum of the
 *     document's labels, match_true = #{i : label_i == prediction_i == 1}, match =
 *     #{i : label_i == prediction_i}.
 *   totals int64 [4]: totals[j] += sum_d doc_counts[d][j] (accumulated: the caller zeroes it
 *     once).  Integer atomic adds: the result does not depend on their order.  No float
 *     atomics anywhere.
 * An empty document gives nsel = 0, a row of -1 and four zeros.
 *
 * Refused documents.  A document with more than n_max rows, or (blocking) with
 * gram_cnt[d] < 0 or > gram_max, or with an id outside [0, gram_cnt[d]) in one of its rows'
 * lists, gets nsel[d] = -1, a row of -1 and zero counts and adds nothing to totals; the
 * other documents of the call are unaffected.  Every id is validated with an unsigned
 * compare before the bitmap is touched: nothing is read or written out of range.
 *
 * HSG_EINVAL before any launch: n < 0, B < 1, m < 0, an (n_max, gram_max) that
 * hsg_eval_select_supported declines, sel_ld below the bound above, a NULL doc_off, sel,
 * nsel, doc_counts or totals, NULL logits or labels with n > 0, gram_ptr without gram_ids or
 * gram_cnt.  n == 0 still writes nsel, sel and doc_counts (every document is empty).
 *
 * Shape: B blocks of one wave.  Scores go to LDS as order-preserving integer keys;
 * rank_i = #{j : key_j precedes key_i} by counting (O(N^2 / 64) per lane); the blocking walk
 * is serial over the ranked candidates with the lanes striding over a candidate's ids, the
 * verdict from a 64-bit ballot, the bits set with LDS integer atomics.  Its cost is the
 * latency of one wave per document, not bandwidth. */
int hsg_eval_select(int n, int B, const float *logits, const int64_t *labels, const int32_t *doc_off, int m,
                    int n_max, const int32_t *gram_ptr, const int32_t *gram_ids, const int32_t *gram_cnt,
                    int gram_max, int32_t *sel, int sel_ld, int32_t *nsel, int32_t *doc_counts, int64_t *totals,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_EVAL_H_ */
