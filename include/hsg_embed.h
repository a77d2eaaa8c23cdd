/*
 * hsg_embed.h -- C ABI of the trainable word embedding (libhsg.so, gfx950): the row lookup
 * of HSumGraph.set_wnfeature (HiGraph.py:144-152) and the dense embedding gradient of
 * `train.py --embed_train` (train.py:342), summed over BOTH uses of the shared nn.Embedding
 * -- the word nodes and the sentence CNN's rows (module/Encoder.py:56-68) -- in one fixed
 * order, without float atomics.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their
 * own (as include/hsg_train.h and include/hsg_model.h).  This header carries the same two
 * obligations itself: its declarations equal its entry in the binding's registry,
 * _lib.ABI["hsg_embed.h"] (tests/test_abi_conformance.py),
 * and every entry point below that writes through a pointer has a guard-band case in
 * tests/test_gpu_embed_guard.py.
 *
 * Conventions are hsg.h's: device pointers, fp32 row-major matrices with explicit row
 * pitches (ld*, in elements, >= the row width), caller-owned workspaces, no allocation,
 * no synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last,
 * every call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any
 * launch (a NULL pointer that is not optional, a base that is not 16-byte aligned, a pitch
 * below the width or no multiple of 4, a negative count, a D that hsg_embed_supported
 * declines).  The embedding table E and its gradient dE are contiguous [V][D].
 */
#ifndef HSG_EMBED_H_
#define HSG_EMBED_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_embed_supported: D a multiple of 4 in [4, 4096] (rows move as 16-byte vectors). */
int hsg_embed_supported(int D);

/* ---- forward: word-node rows ------------------------------------------------------------
 * Xw[i] = E[wid[i]] for i < n_w: bit for bit what nn.Embedding returns.  wid int64 [n_w],
 * Xw [n_w][D] (ldx).  A wid[i] outside [0, V) is never used as an index: row i is NaN.
 * n_w == 0 returns 0 without a launch.  (The CNN's rows keep hsg_cnn_gather.) */
int hsg_embed_rows(int n_w, int V, int D, const int64_t *wid, const float *E, float *Xw, int ldx, void *stream);

/* ---- backward: the dense gradient --------------------------------------------------------
 * An occurrence is a pair (token v, source row s).  Sources are numbered over two
 * matrices: s in [0, n_w) is row s of dW [n_w][D] (ldw), the word nodes' gradient;
 * s = n_w + r is row r of dX [rows][D] (ldx), the gradient of the CNN row matrix in
 * hsg_cnn_gather's layout (a sentence's pad row holds the sum over all its padded
 * positions and counts once, for token 0).
 *
 * occ int64 [n_occ]: the occurrences as keys (v << 32) | s, SORTED ascending (so by
 * token, then by source).  An entry whose token lies outside [0, V) is dropped: it adds
 * nothing and ends the run before it.  That is how the caller drops the occurrences of a
 * padding index -- it replaces their keys by INT64_MAX before sorting, so they sit behind
 * every kept entry and the kept entries' list positions are those of the list without
 * them.  A source outside [0, n_w + rows) is never used as an index: it contributes NaN.
 *
 * Summation order (the contract).  P = hsg_embed_piece_rows() is a compile-time constant
 * of the library (32): it does not depend on the device, the grid or the batch.  Cut the
 * sorted list into aligned chunks [kP, (k+1)P).  The pieces of token v, whose entries
 * are the run [a, b) of the list, are the intersections of the run with the chunks.  Each
 * piece is summed in ascending list position starting FROM its first element (no 0 + in
 * front); the piece sums are then added in ascending order, ((p0 + p1) + p2) + ...; dE[v]
 * is that value.  Every row of dE without a kept occurrence is +0.0.  All arithmetic is
 * fp32 addition: there is no multiply to fuse and no atomic.  Two calls on the same
 * inputs are bitwise equal, whatever the pitches and wherever the buffers lie.
 *
 * hsg_embed_grad clears dE [V][D] on the stream (also when n_occ == 0, after which it
 * returns without a launch), then runs one wave per (chunk, 256 columns): a run inside
 * the chunk is stored straight to dE[v]; the piece of a run that enters the chunk from
 * the left goes to the chunk's head slot, the piece of a run that starts in the chunk and
 * leaves it to the right to its tail slot.  A second launch merges: the wave of the chunk
 * where a crossing run starts adds to its tail slot the head slots of the following
 * chunks while they begin with the same token, in order, and stores dE[v].  A token with
 * n occurrences thus costs n / P row adds in the merge instead of one chain of n.
 *
 * ws: hsg_embed_ws_floats(n_occ, D) = 2 * D * ceil(n_occ / P) floats (host-only query; 0
 * for n_occ <= 0 or an unsupported D), contents undefined afterwards; may be NULL when
 * that is 0.  dW may be NULL when n_w == 0 and dX when rows == 0.  n_occ may be anything
 * in [0, ...): it need not equal n_w + rows.
 *
 * hsg_embed_keys: the UNSORTED keys of one batch, one launch: keys[i] = (token << 32) | i for
 * source i of the n_w + rows sources -- wid int64 [n_w] for the word rows, then the CNN
 * rows of ids int64 [n][L] in hsg_cnn_gather's layout (rowoff int32 [n + 1], rows =
 * rowoff[n]; token 0 for a sentence's pad row).  A token equal to padding_idx (-1: none) or
 * outside [0, 2^31 - 1) gets the dropped key INT64_MAX.  The caller sorts keys (any
 * ascending sort: the kept keys are unique) and hands them to hsg_embed_grad.  Nothing to
 * do (n_w + rows == 0) returns 0 without a launch. */
int hsg_embed_keys(int n_w, int n, int L, long rows, const int64_t *wid, const int64_t *ids, const int32_t *rowoff,
                   long padding_idx, int64_t *keys, void *stream);
int hsg_embed_piece_rows(void);
size_t hsg_embed_ws_floats(long n_occ, int D);
int hsg_embed_grad(int V, int D, long n_occ, const int64_t *occ, int n_w, const float *dW, int ldw, long rows,
                   const float *dX, int ldx, float *dE, float *ws, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_EMBED_H_ */
