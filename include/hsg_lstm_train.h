/*
 * hsg_lstm_train.h -- C ABI of the sentence LSTM's training path around the recurrence
 * kernels of include/hsg.h (hsg_lstm_fwd / hsg_lstm_bwd): the per-step packing of the
 * nn.LSTM parameters into the operands those kernels and the projection GEMM read, and the
 * three weight gradients of a layer as ONE product (libhsg.so, gfx950).  The opt-in path of
 * path_options(HSG_SENT_LSTM="2") behind hetersumgraph_amd.lstm.sent_lstm(..., fused=True).
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their
 * own (as include/hsg_cnn_tokens.h).  This header carries the same two obligations itself:
 * its declarations equal its entry in the binding's registry, _lib.ABI["hsg_lstm_train.h"]
 * (tests/test_abi_conformance.py), and every entry point below that writes through a
 * pointer has a guard-band case in tests/test_gpu_lstm_train_guard.py.
 *
 * Conventions are hsg.h's: device pointers, fp32 row-major matrices, explicit row pitches
 * (ld*, in elements, >= the row width) where a parameter list has one and contiguous
 * otherwise, caller-owned workspaces, no allocation, no synchronisation, no global mutable
 * state, `stream` (a hipStream_t as void*) last, every call graph-capturable; 0 on success,
 * a hipError_t, or HSG_EINVAL before any HIP call (a NULL pointer that is not optional, a
 * base that must be 16-byte aligned and is not, a short pitch, a negative count, a shape
 * hsg_lstm_train_supported declines).
 *
 * Shapes.  hid = 128 hidden units per direction, ndir = 1 or 2, G = 4 * hid gate rows per
 * direction in torch's order (i, f, g, o), M = ndir * G.  Layer 0 reads `in` columns, every
 * later layer ndir * hid.  Rows are the documents' sentences laid end to end: document d
 * owns rows doc_off[d] .. doc_off[d + 1] - 1 (int32 [n_docs + 1], doc_off[0] = 0, ascending,
 * doc_off[n_docs] = n_rows; an empty document is two equal offsets).
 */
#ifndef HSG_LSTM_TRAIN_H_
#define HSG_LSTM_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_lstm_pack takes at most this many layers (its 4 * n_layers * ndir parameter pointers
 * travel in the kernel's arguments, as hsg_train.h's tensor table does). */
#define HSG_LSTM_PACK_MAX_LAYERS 4
/* hsg_lstm_dw cuts the rows into aligned chunks of this many rows (= hsg_lstm_dw_chunk()). */
#define HSG_LSTM_DW_CHUNK 192

/* hsg_lstm_train_supported: hid == 128 (hsg_lstm_supported's), ndir 1 or 2, in > 0 and a
 * multiple of 4. */
int hsg_lstm_train_supported(int hid, int ndir, int in);

/* ---- packed parameters -----------------------------------------------------------------------
 * One buffer holds, layer after layer, the operands of the layer's projection GEMM and of
 * the recurrence, with in_l = in for layer 0 and ndir * hid after it:
 *     W_ih [M][in_l]            rows d * G .. d * G + G - 1 = weight_ih of direction d
 *     W_hh [ndir][G][hid]       = weight_hh of direction d
 *     bias [M]                  = bias_ih + bias_hh, ONE fp32 add per element
 * in this order, each contiguous.  hsg_lstm_pack_layer_offset(layer, ...) is the float
 * offset of layer `layer` (0 for layer 0; a multiple of 4); W_hh lies M * in_l floats and
 * bias M * in_l + M * hid floats behind it.  hsg_lstm_pack_floats(n_layers, ...) is the
 * buffer's length (= the offset of layer n_layers).  Both are host-only queries and return
 * 0 for an unsupported shape, a negative layer or more than HSG_LSTM_PACK_MAX_LAYERS.
 *
 * hsg_lstm_pack: params is a HOST array of 4 * n_layers * ndir device pointers in (layer,
 * direction, weight_ih, weight_hh, bias_ih, bias_hh) order, each contiguous and 16-byte
 * aligned, as is out.  One launch for all layers; every float of out is written exactly
 * once; weights are bit copies.  n_layers >= 1. */
size_t hsg_lstm_pack_layer_offset(int layer, int hid, int ndir, int in);
size_t hsg_lstm_pack_floats(int n_layers, int hid, int ndir, int in);
int hsg_lstm_pack(int n_layers, int hid, int ndir, int in, const float *const *params, float *out, void *stream);

/* ---- the weight gradients of one layer -------------------------------------------------------
 * With dgates [n_rows][M] (contiguous: hsg_lstm_bwd's output), the layer's input x
 * [n_rows][in] (ld_x) and its output h [n_rows][ndir * hid] (ld_h):
 *     dW_ih[m][k]     = sum_r dgates[r][m] * x[r][k]                          [M][in]
 *     dW_hh[d][j][k]  = sum_r dgates[r][d * G + j] * h_prev_d(r)[k]           [ndir][G][hid]
 *     db[m]           = sum_r dgates[r][m]                                    [M]
 * h_prev_0(r) = h[r - 1][0 .. hid) unless r is the first row of its document, h_prev_1(r) =
 * h[r + 1][hid .. 2 hid) unless r is the last row of its document; zero there.  h is read in
 * place: no gathered copy, no zero row; h[r - 1] / h[r + 1] are never read at a document
 * edge, row 0 or row n_rows - 1, whatever doc_off holds.  db is the gradient of bias_ih and
 * of bias_hh alike.
 *
 * Order (the contract).  C = HSG_LSTM_DW_CHUNK is a compile-time constant of the library:
 * it does not depend on the device, the grid or the batch.  The rows are cut into aligned
 * chunks [k C, (k + 1) C); the chunk count ceil(n_rows / C) depends on n_rows alone.  A
 * first launch forms every chunk's partial with exact-fp32 products: each element is one
 * fmaf chain over the chunk's rows in ascending order, starting from +0.0 (the f32-input
 * MFMA v_mfma_f32_16x16x4_f32; nothing is narrowed to bf16); a db partial is four
 * interleaved sums, the rows r = 0, 1, 2, 3 (mod 4) ascending, joined as (s0 + s1) +
 * (s2 + s3).  Rows past n_rows and masked h_prev rows enter as exact zeros.  A second launch
 * inside the same call adds the partials in ascending chunk order, (p0 + p1) + p2 ...  No
 * atomics, no cross-block hand-off, no fence: the result is a pure function of the inputs
 * and two calls are bitwise equal, whatever the pitches and wherever the buffers lie.
 * n_rows == 0 or n_docs == 0 writes +0.0 to every output.
 *
 * One block of four waves owns 128 gate rows x 64 operand columns of one chunk (wave w: 32
 * x 64, eight 16 x 16 accumulators); grid = ceil((ceil16(in) + hid) / 64) x M / 128 x
 * chunks, 336 and 288 blocks for n_rows = 1120, ndir = 2, in = 300 and 256.
 *
 * ws: hsg_lstm_dw_ws_floats(n_rows, ndir, in) = ceil(n_rows / C) * M * (in + hid + 1) floats
 * (host-only query; 0 for n_rows <= 0 or an unsupported shape), contents undefined
 * afterwards; may be NULL when that is 0.  ws, dW_ih, dW_hh and db are 16-byte aligned.
 * n_rows <= 65535 * C. */
int hsg_lstm_dw_chunk(void);
size_t hsg_lstm_dw_ws_floats(int n_rows, int ndir, int in);
int hsg_lstm_dw(int n_docs, int n_rows, int hid, int ndir, int in, const int32_t *doc_off, const float *dgates,
                const float *x, int ld_x, const float *h, int ld_h, float *ws, float *dW_ih, float *dW_hh,
                float *db, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_LSTM_TRAIN_H_ */
