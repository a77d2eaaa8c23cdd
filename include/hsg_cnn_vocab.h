/*
 * hsg_cnn_vocab.h -- C ABI of the sentence CNN's inference forward on a vocabulary product
 * table (libhsg.so, gfx950): the opt-in path of path_options(HSG_SENT_CNN_VOCAB="1") behind
 * hetersumgraph_amd.cnn.sent_cnn_vocab, for a forward that records no gradient
 * (module/Encoder.py:56-76 under model.eval() and torch.no_grad(), as the reference evaluates:
 * train.py:196-200, evaluation.py:78-81).
 *
 * include/hsg_cnn_tokens.h states the identity Y[row] = (E Wall^T)[token] + (P Wall^T)[position].
 * While no parameter changes, both products are constants: TW = [E ; P] Wall^T over the WHOLE
 * vocabulary is built once per evaluation pass (two hsg_gemm_f32 calls, the caller's), and the
 * encoder's forward is then the one launch below, which reads the token ids and gathers TW rows.
 * There is no per-batch mark, scan, table copy, GEMM or read-back.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their own
 * (as include/hsg_cnn_tokens.h).  This header carries the same two obligations itself: its
 * declarations equal its entry in the binding's registry, _lib.ABI["hsg_cnn_vocab.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a pointer
 * has a guard-band case in tests/test_gpu_cnn_vocab_guard.py.
 *
 * Conventions are hsg.h's: device pointers, fp32 row-major matrices with explicit row pitches
 * (ld*, in elements, >= the row width, a multiple of 4), no allocation, no synchronisation, no
 * global mutable state, `stream` (a hipStream_t as void*) last, every call graph-capturable; 0 on
 * success, a hipError_t, or HSG_EINVAL before any launch (a NULL pointer that is not optional, a
 * float base that is not 16-byte aligned, a bad pitch, a negative count, a shape
 * hsg_cnn_vocab_supported declines).  Token 0 is PAD; padding is trailing; ids int64 [n][L];
 * rowoff int32 [n + 1] is hsg_cnn_gather's: len_s = rowoff[s + 1] - rowoff[s] - 1 (clamped to
 * [0, L]).  Columns: q(h, i, c) = tap(h, i) * 50 + c with tap(h, i) = (h - 2)(h + 1) / 2 + i for
 * h = 2..7, i < h, c < 50 (hsg_cnn_taps() = 1350); feat / arg are contiguous [n][300], column
 * (h - 2) * 50 + c.
 */
#ifndef HSG_CNN_VOCAB_H_
#define HSG_CNN_VOCAB_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_cnn_vocab_supported: 7 <= L <= 400 (a sentence's token numbers are staged in LDS). */
int hsg_cnn_vocab_supported(int L);

/* ---- forward: shifted sum, ReLU, max-pool with first argmax ----------------------------------
 * TW [V + Pn][>= 1350] (ldtw): rows 0 .. V - 1 are E Wall^T, row V + p is P[p] Wall^T (row V = the
 * padding position); Pn >= L + 1 is the caller's business.  Same outputs and tie rule as
 * hsg_cnn_pool, and the value contract of hsg_cnn_tok_pool with U = V and the identity slot map:
 * the windows t = 0 .. min(len_s, L - h + 1) - 1 are scanned ascending, then -- when len_s < L - h
 * + 1 -- the all-padding window once, at t = len_s; the first maximum by strict > wins;
 * feat = max(best, 0), arg = its t.  Value of window t, fp32, unfused, in this order:
 *     v = b_h[c];  for i = 0..h-1:  v = v + (TW[tok(s, t+i)][q(h,i,c)] + TW[V + pos(s, t+i)][q(h,i,c)])
 * with tok(s, r) = ids[s][r], pos(s, r) = r + 1 for r < len_s, else 0 and 0.  An id outside [0, V)
 * is read as PAD (the caller checks the range where it builds the layout).  bias: six device
 * pointers (host array), b_h [50].
 *
 * Rows are read whole, as 16-byte vectors (so ldtw % 4 == 0 and TW 16-byte aligned, and the up to
 * ldtw - 1350 pad columns of a row may be read; they are never used).  The schedule -- tiles of
 * consecutive positions summed into LDS, windows carried in registers across tiles -- does not
 * enter the values: two calls are bitwise equal, whatever the pitch and wherever the buffers lie.
 * n == 0 returns 0 and writes nothing. */
int hsg_cnn_vocab_pool(int n, int L, int V, const int64_t *ids, const int32_t *rowoff, const float *TW, int ldtw,
                       const float *const *bias, float *feat, int32_t *arg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_CNN_VOCAB_H_ */
