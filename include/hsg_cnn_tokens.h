/*
 * hsg_cnn_tokens.h -- C ABI of the sentence CNN on distinct tokens and of its sparse weight
 * gradient (libhsg.so, gfx950): the opt-in paths of path_options(HSG_SENT_CNN="dw" |
 * "tokens") behind hetersumgraph_amd.cnn.sent_cnn_tokens, for a FROZEN word embedding and
 * position table (module/Encoder.py:56-76 with the reference's default embed_train=False).
 *
 * The convolution is linear and X[row] = E[token] + P[position], so
 *     Y[row] = (E Wall^T)[token] + (P Wall^T)[position]:
 * the GEMM needs one row per DISTINCT token of the batch plus L + 1 position rows instead
 * of one row per token occurrence (hsg_cnn_tok_mark / _table build that operand, the
 * existing hsg_gemm_f32 multiplies it, hsg_cnn_tok_pool is hsg_cnn_pool on the two-row
 * sums).  The weight gradient dWall = dY^T X multiplies a dY that has one non-zero window
 * per (sentence, height, channel); hsg_cnn_tok_dw sums those windows directly, without dY,
 * the saved X or a GEMM.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their
 * own (as include/hsg_embed.h).  This header carries the same two obligations itself: its
 * declarations equal its entry in the binding's registry, _lib.ABI["hsg_cnn_tokens.h"]
 * (tests/test_abi_conformance.py), and every entry
 * point below that writes through a pointer has a guard-band case in
 * tests/test_gpu_cnn_tokens_guard.py.
 *
 * Conventions are hsg.h's: device pointers, fp32 row-major matrices with explicit row
 * pitches (ld*, in elements, >= the row width, a multiple of 4), caller-owned workspaces, no
 * allocation, no synchronisation, no global mutable state, `stream` (a hipStream_t as void*)
 * last, every call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any
 * launch (a NULL pointer that is not optional, a float base that is not 16-byte aligned, a
 * bad pitch, a negative count, a shape hsg_cnn_tok_supported declines).  E [V][D] and
 * P [L + 1][D] (row 0 = the padding position) are contiguous.  Token 0 is PAD; padding is
 * trailing; ids int64 [n][L]; rowoff int32 [n + 1] is hsg_cnn_gather's: len_s =
 * rowoff[s + 1] - rowoff[s] - 1 (clamped to [0, L]).  Columns: q(h, i, c) = tap(h, i) * 50 + c
 * with tap(h, i) = (h - 2)(h + 1) / 2 + i for h = 2..7, i < h, c < 50 (hsg_cnn_taps() = 1350);
 * feat / arg / dfeat are contiguous [n][300], column (h - 2) * 50 + c.
 */
#ifndef HSG_CNN_TOKENS_H_
#define HSG_CNN_TOKENS_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_cnn_tok_supported: 7 <= L <= 400 (a sentence's rows are staged in LDS) and D a multiple
 * of 4 in [4, 4096] (rows move as 16-byte vectors). */
int hsg_cnn_tok_supported(int L, int D);

/* ---- the distinct tokens of a batch ---------------------------------------------------------
 * present int32 [V] and bad int32 [1] are zeroed by the caller.  Sets present[0] = 1 (PAD is
 * always a row) and present[v] = 1 for every id v of ids (plain stores of the same value: a
 * benign race).  An id outside [0, V) sets *bad = 1 and writes nothing else.  V >= 1; n == 0
 * still sets present[0].
 *
 * The caller turns present into the slot map slot[v] = (inclusive prefix sum of present)[v] -
 * 1, int32 [V], and U = slot[V - 1] + 1: slots ascend with the token id. */
int hsg_cnn_tok_mark(int n, int L, int V, const int64_t *ids, int32_t *present, int32_t *bad, void *stream);

/* Tb [U + L + 1][D] (ldt): row slot[v] = E[v] for every v with present[v] != 0 and slot[v] in
 * [0, U); row U + p = P[p] for p = 0..L.  Bit copies.  With a slot map as above every row of
 * Tb is written exactly once. */
int hsg_cnn_tok_table(int V, int D, int U, int L, const int32_t *present, const int32_t *slot, const float *E,
                      const float *P, float *Tb, int ldt, void *stream);

/* ---- forward: shifted sum, ReLU, max-pool with first argmax ----------------------------------
 * TW [U + L + 1][>= 1350] (ldtw) = Tb Wall^T.  Same outputs and tie rule as hsg_cnn_pool: the
 * windows t = 0 .. min(len_s, L - h + 1) - 1 are scanned ascending, then -- when len_s < L - h
 * + 1 -- the all-padding window once, at t = len_s; the first maximum by strict > wins;
 * feat = max(best, 0), arg = its t.  Value of window t, fp32, unfused, in this order:
 *     v = b_h[c];  for i = 0..h-1:  v = v + (TW[slot(s, t+i)][q(h,i,c)] + TW[U + pos(s, t+i)][q(h,i,c)])
 * with slot(s, r) = slot[ids[s][r]], pos(s, r) = r + 1 for r < len_s, else slot[0] and 0.  An id
 * outside [0, V) is read as PAD and a slot outside [0, U) as slot 0 (neither occurs behind
 * hsg_cnn_tok_mark's check).  bias: six device pointers (host array), b_h [50]. */
int hsg_cnn_tok_pool(int n, int L, int V, int U, const int64_t *ids, const int32_t *rowoff, const int32_t *slot,
                     const float *TW, int ldtw, const float *const *bias, float *feat, int32_t *arg, void *stream);

/* ---- backward: the sparse weight gradient ----------------------------------------------------
 * g[s][h][c] = dfeat where feat > 0, else 0.  x(s, r)[d] = E[ids[s][r]][d] + P[r + 1][d] for
 * 0 <= r < len_s, else E[0][d] + P[0][d] (one fp32 add; every arg + i goes through this rule
 * before it indexes anything; an id outside [0, V) gives NaN, it is never used as an index).
 *     dWall[q(h,i,c)][d] = sum_s g[s][h][c] * x(s, arg[s][h][c] + i)[d]     [1350][D] (lddw)
 *     dbias[(h-2)*50 + c] = sum_s g[s][h][c]                                  [300]
 *
 * Summation order (the contract).  C = hsg_cnn_tok_chunk() is a compile-time constant of the
 * library (64): it does not depend on the device, the grid or the batch.  The sentences are
 * cut into aligned chunks [kC, (k+1)C).  Each chunk's partial starts from +0.0 and adds its
 * sentences in ascending order as acc = acc + g * x, the multiply and the add rounded
 * separately (acc = acc + g for dbias); the partials are then added in ascending chunk order,
 * (p0 + p1) + p2 ...  Pairs with g == 0 are skipped (they would add exact zeros).  No float
 * atomics.  Two calls on the same inputs are bitwise equal, whatever the pitch and wherever
 * the buffers lie.  n == 0 writes +0.0 everywhere.
 *
 * One block per (chunk, 16 columns of D) stages each sentence's x tile in LDS once and keeps
 * its [1350][16] partial in registers; a second launch adds the partials.
 *
 * ws: hsg_cnn_tok_dw_ws_floats(n, D) = ceil(n / C) * (1350 * D + 300) floats (host-only query;
 * 0 for n <= 0 or an unsupported D), contents undefined afterwards; may be NULL when that is 0. */
int hsg_cnn_tok_chunk(void);
size_t hsg_cnn_tok_dw_ws_floats(int n, int D);
int hsg_cnn_tok_dw(int n, int L, int V, int D, const int64_t *ids, const int32_t *rowoff, const float *E,
                   const float *P, const float *feat, const int32_t *arg, const float *dfeat, float *ws,
                   float *dWall, int lddw, float *dbias, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_CNN_TOKENS_H_ */
