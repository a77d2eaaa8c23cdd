/*
 * hsg_model.h -- C ABI of the model glue (libhsg.so, gfx950): what HSumGraph /
 * HSumDocGraph compute between the two sentence encoders and the WSWGAT stack, and
 * between the stack and the loss (HiGraph.py:96, 108, 130-132, 141, 160, 202, 207,
 * 219-227, 231-244).
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their
 * own (as include/hsg_train.h), and this header carries the same two obligations: its
 * declarations equal its entry in the binding's registry, _lib.ABI["hsg_model.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a
 * pointer has a guard-band case in tests/test_gpu_model_guard.py.
 *
 * Conventions are hsg.h's: device pointers, fp32 row-major matrices with explicit row
 * pitches (ld*, in elements, >= the row width), caller-owned workspaces, no allocation,
 * no synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last,
 * every call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any
 * launch (a NULL pointer that is not optional, a pitch below the width, a negative count,
 * dimensions the *_supported query declines).  A zero row count returns 0 without a
 * launch.  Weights are contiguous nn.Linear matrices [out][in].  There are no float
 * atomics; every sum over rows runs in one fixed order, so two runs are bitwise equal.
 * All arithmetic is fp32, whatever the GEMM mode: a dot product is fmaf chains over 32
 * consecutive k whose sums are added in ascending k.
 */
#ifndef HSG_MODEL_H_
#define HSG_MODEL_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sentence features (HiGraph.py:130-132, 141, 160, 96) ------------------------------
 * Replaces the position-embedding lookup + add + cnn_proj, lstm_proj, the cat of the two
 * and n_feature_proj.  With x = ngram + P[pos]:
 *     F = [ x Wc^T + bc | L Wl^T + bl ]   [n][2*Fn]
 *     S = F Wn^T                          [n][Hs]
 *   ngram [n][E] (ldn), pos int64 [n], P [n_pos][E] contiguous, L [n][Lw] (ldl: may be a
 *   strided view), Wc [Fn][E], bc [Fn], Wl [Fn][Lw], bl [Fn], Wn [Hs][2*Fn].
 * hsg_sentfeat_supported: Fn == 128, Hs == 64, E and Lw multiples of 4 in [4, 512] (the
 * reference defaults E 300, Lw 256, and the unidirectional Lw 128).  The three weight
 * pointers must be 16-byte aligned (HSG_EINVAL otherwise).
 * hsg_sentfeat_rows: the rows of one block (4): ceil(n / 4) blocks of 256 threads, so a
 * 1,120-row batch gives 280 blocks.
 * hsg_sentfeat_fwd: one launch.  Writes S [n][Hs] (lds), F [n][2*Fn] (ldf) and, when X is
 * not NULL, x [n][E] (ldx) for the backward.  A pos[i] outside [0, n_pos) is never used
 * as an index: row i of x, the first Fn columns of row i of F and row i of S are NaN
 * (train.py:121 trips); every other row is unaffected.
 * hsg_sentfeat_bwd: one row-parallel launch.  Given dS [n][Hs] (ldds) writes
 * dF = dS Wn [n][2*Fn] (lddf; its column sums are dbc | dbl, and dWn = dS^T F,
 * dWc = dF[:, :Fn]^T x, dWl = dF[:, Fn:]^T L are the caller's weight-gradient GEMMs) and,
 * where the pointer is not NULL, dngram = dF[:, :Fn] Wc [n][E] (lddn) and
 * dL = dF[:, Fn:] Wl [n][Lw] (lddl). */
int hsg_sentfeat_supported(int E, int Fn, int Lw, int Hs);
int hsg_sentfeat_rows(void);
int hsg_sentfeat_fwd(int n, int E, int Fn, int Lw, int Hs, int n_pos, const float *ngram, int ldn,
                     const int64_t *pos, const float *P, const float *L, int ldl, const float *Wc, const float *bc,
                     const float *Wl, const float *bl, const float *Wn, float *X, int ldx, float *F, int ldf,
                     float *S, int lds, void *stream);
int hsg_sentfeat_bwd(int n, int E, int Fn, int Lw, int Hs, const float *dS, int ldds, const float *Wc,
                     const float *Wl, const float *Wn, float *dF, int lddf, float *dngram, int lddn, float *dL,
                     int lddl, void *stream);

/* ---- doc-node initial state (HiGraph.py:231-244, 202, 207) -----------------------------
 * Replaces the segment mean of set_dnfeature (index_add), dn_feature_proj, the cat of
 * sentence and doc rows and the supernode gather.  One launch writes the whole
 * init [n_super][Hs] (ldi):
 *   super_src int32 [n_super]: v >= 0: the row is sentence v, a copy of S[v];
 *     v < 0: the row is doc d = -(v + 1): (mean of its sentences' S rows) Wd^T, where the
 *     mean is inv_cnt[d] * the sum of S[doc_sent[e]] for e = doc_ptr[d] .. doc_ptr[d+1]-1
 *     in ascending e (the CSR form of the sentence->doc pair list, duplicates kept).
 *   S [n_s][Hs] (lds), doc_ptr int32 [n_docs + 1], doc_sent int32 [pairs], inv_cnt
 *   [n_docs], Wd [Hs][Hs].  Every doc must own exactly one row of super_src.
 * Also writes mean [n_docs][Hs] (contiguous) for the backward.  An index outside its
 * range is never used: the row it feeds becomes NaN.
 * hsg_docinit_supported: Hs == 64.
 * hsg_docinit_bwd: one launch.  Given dInit [n_super][Hs] (ldd):
 *   dS[s] = dInit[sent_row[s]] + sum over e = sent_ptr[s] .. sent_ptr[s+1]-1, ascending,
 *           of inv_cnt[d] * (dInit[doc_row[d]] Wd), d = sent_doc[e]   (the CSC form);
 *   dWd   = sum over docs d ascending of dInit[doc_row[d]]^T mean[d].
 *   sent_row int32 [n_s] and doc_row int32 [n_docs]: the super row of a sentence / doc
 *   (a negative sent_row: the sentence is no supernode and that term is 0).
 * dS [n_s][Hs] (ldds) and dWd [Hs][Hs] may each be NULL (not wanted). */
int hsg_docinit_supported(int Hs);
int hsg_docinit_fwd(int n_s, int n_docs, int n_super, int Hs, const float *S, int lds, const int32_t *super_src,
                    const int32_t *doc_ptr, const int32_t *doc_sent, const float *inv_cnt, const float *Wd,
                    float *mean, float *init, int ldi, void *stream);
int hsg_docinit_bwd(int n_s, int n_docs, int n_super, int Hs, const float *dInit, int ldd,
                    const int32_t *sent_row, const int32_t *doc_row, const int32_t *sent_ptr,
                    const int32_t *sent_doc, const float *inv_cnt, const float *Wd, const float *mean, float *dS,
                    int ldds, float *dWd, void *stream);

/* ---- sentence logits (HiGraph.py:108, 219-227) ------------------------------------------
 * Replaces wh, and for HDSG the two supernode gathers and the per-sentence concat in
 * front of it (the [n][2*Hs] matrix is never formed).
 *   HSG  (sent_super == doc_super == NULL, n_super == n): logits = state Wh^T + bh,
 *        Wh [2][Hs];
 *   HDSG: logits_i = Wh[:, :Hs] state[sent_super[i]] + Wh[:, Hs:] state[doc_super[i]] + bh,
 *        Wh [2][2*Hs], sent_super / doc_super int32 [n] (both or neither).
 *   state [n_super][Hs] (ldst), bh [2], logits [n][2] contiguous.  A row's two sums are 16
 *   lanes' chains joined by a fixed xor tree, kept in double (where a product of two floats
 *   is exact) and rounded to fp32 once after the bias: the nearest fp32 to the exact value
 *   but for double's own rounding.  An index outside [0, n_super) is never used: that
 *   row's logits are NaN.
 * hsg_logits_supported: Hs a multiple of 4 in [4, 256].
 * hsg_logits_bwd_blocks (host-only): the partial rows of ws, ceil(n / 64).
 * hsg_logits_bwd: given dlogits [n][2] writes
 *   dstate [n_super][Hs] (ldd, may be NULL): HSG: row i = dlogits_i Wh.  HDSG: row r gets
 *     dlogits_i Wh[:, :Hs] for the sentence i = sup_sent[r] (int32 [n_super], -1: none)
 *     plus the sum over e = sup_ptr[r] .. sup_ptr[r+1]-1, ascending, of
 *     dlogits_i Wh[:, Hs:], i = sup_list[e] (the inverse list of doc_super; int32
 *     [n_super + 1] and [n]); a row nothing refers to is 0;
 *   dWh [2][W] and dbh [2] (W = Hs or 2*Hs; both or neither, with ws): two-stage sums,
 *     ws [hsg_logits_bwd_blocks(n)][2*W + 2] holds the per-64-row partials (rows
 *     ascending inside a block), then one block adds the partials in ascending order. */
int hsg_logits_supported(int Hs);
int hsg_logits_fwd(int n, int Hs, int n_super, const float *state, int ldst, const int32_t *sent_super,
                   const int32_t *doc_super, const float *Wh, const float *bh, float *logits, void *stream);
int hsg_logits_bwd_blocks(int n);
int hsg_logits_bwd(int n, int Hs, int n_super, const float *dlogits, const float *state, int ldst,
                   const int32_t *sent_super, const int32_t *doc_super, const int32_t *sup_sent,
                   const int32_t *sup_ptr, const int32_t *sup_list, const float *Wh, float *dstate, int ldd,
                   float *ws, float *dWh, float *dbh, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_MODEL_H_ */
