/*
 * hsg_eval_words.h -- C ABI of the evaluation step's sentence selection with n-gram blocking
 * on WORD ids (libhsg.so, gfx950).  It computes what include/hsg_eval.h's hsg_eval_select
 * computes -- per document the top-m selection of Tester.py:105-140 with or without n-gram
 * blocking (Tester.py:155-184), the m == 0 rule (Tester.py:120-122) and the four match
 * counters (Tester.py:133-137), in ONE launch per batch and without a host round trip -- from
 * another blocking operand: the document-local word ids of every sentence.  The device forms
 * the n-gram windows itself and keeps the chosen sentences' windows in an exact hash set in
 * LDS.  Word ids depend neither on the window length nor on m, so they can be made once per
 * example (or in the DataLoader workers); the host does no n-gram work at all.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their own
 * (as hsg_train.h, hsg_model.h, hsg_embed.h and hsg_eval.h).  This header carries the same two
 * obligations itself: its declarations equal its entry in the binding's registry,
 * _lib.ABI["hsg_eval_words.h"] (tests/test_abi_conformance.py),
 * and every entry point below that writes through a pointer has a guard-band case in
 * tests/test_gpu_eval_words_guard.py.
 *
 * Conventions are hsg.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.
 */
#ifndef HSG_EVAL_WORDS_H_
#define HSG_EVAL_WORDS_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_eval_words_supported (host-only): 1 <= n_max <= 1024, 1 <= n_win <= 8, and tab_cap a
 * power of two in [64, 8192] (a table of at most 32 KB in LDS, beside the 12 KB of scores,
 * order and selection flags). */
int hsg_eval_words_supported(int n_max, int n_win, int tab_cap);

/* ---- selection, one wavefront per document ------------------------------------------------
 * Inputs.
 *   logits [n][2] fp32 contiguous; labels int64 [n], the class of each row.
 *   doc_off int32 [B+1]: document d owns rows doc_off[d] .. doc_off[d+1]-1, N_d of them
 *     (offsets are clamped to [0, n], as in hsg_doc_ce); "local index" means row - doc_off[d].
 *   m >= 0: sentences to choose per document (0: the argmax rule below).
 *   n_max: the largest document the caller admits (sizes the LDS arrays).
 *   n_win: the n-gram length in words.
 *   word_ptr int32 [n+1] or NULL (no blocking): the words of row i are
 *     word_ids[word_ptr[i] .. word_ptr[i+1]).  word_ids holds word_ptr[n] entries; every
 *     word_ptr value is clamped to [0, word_ptr[n]] and an end below its start is an empty
 *     sentence, so nothing outside word_ids is read whatever word_ptr holds.  Word ids are
 *     arbitrary int32 values: they are only compared with each other, so no id is invalid.
 *   tab_cap: the number of slots of the seen set (sizes the table in LDS).
 *
 * Windows.  A sentence of len words has the windows t = 0 .. len - n_win - 1, window t being
 * the n_win consecutive ids from position t: the reference never uses a sentence's last
 * n-gram (Tester.py:170).  A sentence of at most n_win words has no window.
 *
 * Candidate order (m > 0).  Candidates are ordered by logits[i][1] descending AS FLOATS:
 * -0.0 == 0.0; NaN is greater than every number (where torch puts it) and all NaNs are
 * equal; equal keys are ordered by ascending local index.  This is a total order.  It is
 * this project's rule, not the reference's, whose order among equal scores is whatever
 * torch.sort / torch.topk happen to return.
 *
 * Selection without blocking (m > 0, word_ptr == NULL): the first k = min(m, N_d) candidates
 * of that order.
 *
 * Selection with blocking (m > 0, word_ptr != NULL), Tester.py:155-184: walk the candidates
 * in order; skip a candidate if one of its windows equals, id for id, a window of an already
 * chosen sentence; otherwise choose it and add all its windows to the document's seen set;
 * stop once k are chosen or the candidates run out (fewer than k may survive).  Windows of a
 * skipped sentence are not added.  A sentence's own repeated windows do not block it (all
 * its windows are tested first, then inserted).  A sentence without windows is never blocked.
 *
 * Selection for m == 0 (Tester.py:120-122): row i is selected iff argmax(logits[i]) != 0
 * with torch's NaN rule, i.e. iff !isnan(p0) && (isnan(p1) || p1 > p0); selected rows are
 * written in ascending index order.  Blocking is ignored, as in the reference: word_ptr and
 * word_ids are not read and only the n_max refusal below applies.
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
 * Refused documents.  A document with more than n_max rows is refused.  With blocking, a
 * document is also refused if choosing a sentence would bring the number of windows stored
 * for it above tab_cap.  Windows are counted WITH repeats -- every chosen sentence
 * contributes len - n_win if that is positive, else zero -- and the count is checked before
 * anything is inserted, so the rule does not depend on whether equal windows share a slot.  A
 * refused document gets nsel[d] = -1, a row of -1 and zero counts and adds nothing to totals;
 * the other documents of the call are unaffected.
 *
 * HSG_EINVAL before any launch: n < 0, B < 1, m < 0, an (n_max, n_win, tab_cap) that
 * hsg_eval_words_supported declines (with or without blocking), sel_ld below the bound above,
 * a NULL doc_off, sel, nsel, doc_counts or totals, NULL logits or labels with n > 0, word_ptr
 * without word_ids.  n == 0 still writes nsel, sel and doc_counts (every document is empty).
 *
 * Shape: B blocks of one wave.  Scores go to LDS as order-preserving integer keys;
 * rank_i = #{j : key_j precedes key_i} by counting (O(N^2 / 64) per lane); the blocking walk
 * is serial over the ranked candidates with the lanes striding over a candidate's windows and
 * the verdict from a 64-bit ballot.  The seen set is an open-addressing table of tab_cap
 * int32 slots in LDS; a slot holds the position in word_ids of a stored window's first word
 * (-1: free).  Membership is decided by comparing the n_win ids, never by the hash alone;
 * equal windows share a slot; slots are claimed with an LDS integer compare-and-swap; every
 * probe loop is bounded by tab_cap steps.  Its cost is the latency of one wave per document,
 * not bandwidth. */
int hsg_eval_select_words(int n, int B, const float *logits, const int64_t *labels, const int32_t *doc_off, int m,
                          int n_max, int n_win, const int32_t *word_ptr, const int32_t *word_ids, int tab_cap,
                          int32_t *sel, int sel_ld, int32_t *nsel, int32_t *doc_counts, int64_t *totals,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_EVAL_WORDS_H_ */
