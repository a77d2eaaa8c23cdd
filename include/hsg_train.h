/*
 * hsg_train.h -- C ABI of the training-step tail (libhsg.so, gfx950): the per-document
 * loss, the gradient norm, and clip + Adam (train.py:115-119, 132-135).
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, but in a header of
 * their own.  Every public header carries the same two obligations: its declarations
 * equal, name by name and parameter by parameter, its entry in the binding's registry
 * (_lib.ABI["hsg_train.h"]; tests/test_abi_conformance.py), and every entry point below
 * that writes through a pointer has a guard-band case, here in
 * tests/test_gpu_train_guard.py (tests/test_guard_coverage.py does this for hsg.h).
 *
 * Conventions are hsg.h's: device pointers unless said otherwise, caller-owned
 * workspaces, no allocation, no synchronisation, no global mutable state, `stream` (a
 * hipStream_t as void*) last, every call graph-capturable; 0 on success, a hipError_t,
 * or HSG_EINVAL before any launch.
 */
#ifndef HSG_TRAIN_H_
#define HSG_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-document cross entropy (train.py:115-119) ------------------------------------
 * Replaces filter_nodes + label gather + CrossEntropyLoss(reduction='none') + the node
 * column write + dgl.sum_nodes + mean with two launches: one block per document, then a
 * one-block finish.
 *   logits [n][C] fp32, contiguous.  C must be 2 (HSG_EINVAL otherwise).
 *   labels, two forms:
 *     rows == NULL: labels is int64 [n], the class of each row (L and N are ignored);
 *     rows != NULL: labels is the node label matrix int64 [N][L], rows is int64 [n] (the
 *       sentence node ids) and label_i = sum_j labels[rows[i]][j]  (train.py:116).
 *   doc_off int32 [B+1]: document d owns rows doc_off[d] .. doc_off[d+1]-1; doc_off[0] = 0
 *     and doc_off[B] = n (offsets are clamped to [0, n]; a row no document owns is not
 *     written).  B >= 1.  A document without rows contributes 0.
 * Writes row_loss [n], doc_loss [B] (sum over the document's rows), mean [1]
 * (sum_d doc_loss[d] / B) and dlogits [n][C] = (softmax - onehot) / B, the gradient of
 * mean.  The loss is softplus(z_other - z_label) and the gradient +-sigmoid of the same
 * difference: no overflow at |logit| = 100, ln 2 at a tie.  A label outside [0, C), or a
 * rows[i] outside [0, N), gives that row a NaN loss (so its document's sum and the mean
 * are NaN: train.py:121 trips) and a zero gradient row; nothing is read out of range.
 * Every sum runs in a fixed order (a thread's rows ascending, then a fixed tree); there
 * are no float atomics: two runs are bitwise equal. */
int hsg_doc_ce(int n, int C, int B, const float *logits, const int64_t *labels, int L, int64_t N,
               const int64_t *rows, const int32_t *doc_off, float *row_loss, float *doc_loss, float *mean,
               float *dlogits, void *stream);

/* ---- multi-tensor gradient norm, clip and Adam (train.py:132-135) -----------------------
 * Replaces clip_grad_norm_ over the parameter list and torch.optim.Adam.step with two
 * kinds of launch over a HOST array of descriptors, one per parameter tensor (fp32,
 * contiguous, n elements; n == 0 is skipped).  The library copies up to
 * hsg_mt_tensors_per_launch() = 64 descriptors plus their block offsets into the kernel
 * arguments BY VALUE (2,824 bytes; 2,840 / 2,864 with the two kernels' other explicit
 * arguments, of the 4,096 a dispatch may carry), so there is no device-side table and no
 * copy, and a captured graph node holds the table.  T descriptors take ceil(T / 64)
 * launches of each kernel.  A
 * 256-thread block owns one chunk of hsg_mt_chunk() = 4,096 consecutive elements of one
 * tensor (thread t the 4-element groups t, t + 256, t + 512, t + 768 of the chunk); it
 * uses 16-byte accesses when every pointer of the tensor that the mode touches is
 * 16-byte aligned and 4-byte accesses otherwise (views at odd element offsets of a flat
 * buffer); the arithmetic and its order are the same in both, so results do not depend on
 * the layout.
 *
 * hyper: device double [8] = { lr, beta1, beta2, eps, weight_decay, max_norm (< 0:
 * clipping off), step, reserved }.  The hyper-parameters are read on the device at run
 * time, so a captured graph follows a host-side change that the caller copies in
 * (train.py:150-153, lr_descent).
 *
 *   hsg_mt_blocks (host-only): the number of blocks = partials = sum_i ceil(n_i / 4096).
 *     0 for T == 0; (size_t)-1 for an invalid table (n < 0, a NULL g with n > 0, or more
 *     than 2^31 - 1 blocks).
 *   hsg_mt_sqnorm: partials[b] = the sum of g^2 over block b's chunk (fp32, a fixed order;
 *     blocks numbered through the table in order).  partials is float [hsg_mt_blocks].
 *     The first launch also advances the step counter, hyper[6] += 1 (as hsg_seed_advance
 *     does for the dropout seed), so a replayed graph sees fresh bias corrections; hyper
 *     may be NULL (a stand-alone norm: nothing is advanced).  Only g and n are read.
 *     The squares and their sums are fp32: a finite |g| above about 1.8e19 overflows its
 *     partial to inf, so the norm is inf and the clip coefficient 0 -- as torch's fp32
 *     vector_norm overflows.  A NaN or inf gradient element makes the norm NaN or inf.
 *   hsg_mt_adam: every block sums ALL partials in double in one fixed order (thread t
 *     the partials t, t + 256, ... ascending, then a fixed tree) -- the same total in
 *     every block, so there is no inter-workgroup hand-off and no fence (a strict
 *     index-order chain would serialise the double adds in every block; its cost was
 *     estimated at about 2 us per block, not measured) -- and forms
 *     norm = sqrt(total), coef = max_norm / (norm + 1e-6) clamped at 1 (NaN stays NaN, as
 *     torch's clamp), coef = 1 when max_norm < 0.  Then with g' = coef * g and
 *     t = hyper[6], torch.optim.Adam's update:
 *       g' += weight_decay * p;  m += (g' - m) * (1 - beta1);
 *       v = beta2 * v + (1 - beta2) * g'^2;
 *       p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *     g is const: .grad is never rewritten.  scale_only != 0: instead p[i] = coef * g[i]
 *     for every tensor (m, v and all of hyper but max_norm unused; p may equal g: the
 *     stand-alone clip_grad_norm_).  norm_out (float [1], may be NULL) receives norm.
 *     T == 0 launches nothing and writes nothing. */
struct hsg_mt_tensor {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t n;
};
int hsg_mt_tensors_per_launch(void);
int hsg_mt_chunk(void);
size_t hsg_mt_blocks(const struct hsg_mt_tensor *tensors, int T);
int hsg_mt_sqnorm(const struct hsg_mt_tensor *tensors, int T, float *partials, double *hyper, void *stream);
int hsg_mt_adam(const struct hsg_mt_tensor *tensors, int T, const float *partials, const double *hyper,
                int scale_only, float *norm_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_TRAIN_H_ */
