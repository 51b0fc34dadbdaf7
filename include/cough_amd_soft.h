/*
 * cough_amd_soft.h -- C-ABI of libcough_amd_soft.so, the companion of libcough_amd.so that trains on soft targets: the
 * three training steps of cough_amd.h with a batch's targets given as class probabilities (MixUp's mixed one-hot labels,
 * label smoothing, a teacher's probabilities) instead of class indices, and the MixUp of a batch in one launch.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and the five other companions at version 1 with theirs, so
 * these entry points are exported from a seventh library with a version of its own.  The conventions are those of
 * cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E*
 * code of cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on
 * `stream` (a hipStream_t; NULL = default stream); no call allocates, copies from the host or synchronises; every
 * argument is checked before the launch; no kernel uses atomics, so the same input gives the same bits.
 *
 * THE SOFT-TARGET LOSS.  torch's F.cross_entropy(z, y, weight=w) for a floating y of shape (B, 2), reduction "mean":
 *   per clip   l_b = -(w0 y_b0 lp_b0 + w1 y_b1 lp_b1),  lp_b = log_softmax(z_b),  w = (1, 1) without class weights
 *   loss       sum of l_b over the batch / B          -- the batch size, NOT the sum of the weights as with class indices
 *   dlogits    dz_bc = (softmax(z_b)_c S_b - w_c y_bc) / B,  S_b = w0 y_b0 + w1 y_b1
 * A row need not sum to 1 and a row of zeros contributes nothing; the values are not validated (that would need a
 * synchronisation), and a NaN in a row gives a NaN loss, as torch does.  Everything else of a step -- the forward pass, the
 * dropout draws, the fixed-order loss reduction, the non-finite guard, every gradient behind dlogits, the BatchNorm
 * running statistics -- is the step of cough_amd.h: the same kernels, compiled from the same source.  For one-hot rows
 * without class weights a soft step therefore equals the class-index step bit for bit.
 */
#ifndef COUGH_AMD_SOFT_H
#define COUGH_AMD_SOFT_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_soft_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_SOFT_ABI_VERSION 1

int cough_soft_abi_version(void);
const char* cough_soft_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ the three training steps on soft targets
 * cough_train_forward_backward, cough_train_small_forward_backward and cough_train_std_forward_backward of cough_amd.h,
 * argument for argument, with d_soft_targets ([n_clips][2] float32, row-major: the probabilities of class 0 and 1) in
 * place of d_targets.  The workspace is the hard step's: size it with cough_train_workspace_bytes,
 * cough_train_small_workspace_bytes and cough_train_std_workspace_bytes of cough_amd.h.  The argument checks are the hard
 * step's too (NULL arguments, shapes, dropout probabilities, BatchNorm momentum / eps, the workspace). */
int cough_train_forward_backward_soft(const float* d_x, int n_clips, int height, int width, const float* d_soft_targets,
                                      const float* d_class_weights, const float* d_dropout_mask, unsigned long long seed,
                                      unsigned long long offset, float p, const float* d_params, float* d_grads,
                                      float* d_running, long long* d_num_batches, float momentum, float eps, float* d_loss,
                                      float* d_logits, float* d_mask_out, void* d_workspace, size_t workspace_bytes,
                                      void* stream);
int cough_train_small_forward_backward_soft(const float* d_x, int n_clips, int height, int width,
                                            const float* d_soft_targets, const float* d_class_weights,
                                            const float* d_dropout_mask, unsigned long long seed, unsigned long long offset,
                                            float p, const float* d_params, float* d_grads, float* d_running,
                                            long long* d_num_batches, float momentum, float eps, float* d_loss,
                                            float* d_logits, float* d_mask_out, void* d_workspace, size_t workspace_bytes,
                                            void* stream);
int cough_train_std_forward_backward_soft(const float* d_x, int n_clips, int height, int width, const float* d_soft_targets,
                                          const float* d_class_weights, const float* d_dropout_mask,
                                          unsigned long long seed, unsigned long long offset, float p_block, float p_fc,
                                          const float* d_params, float* d_grads, float* d_running, long long* d_num_batches,
                                          float momentum, float eps, float* d_loss, float* d_logits, float* d_mask_out,
                                          void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ MixUp of a batch with a permutation of itself
 * One launch for MixUp.mix_batch: two cough_mix_rows calls (images, labels) and a one-hot.
 *   d_x       [n_rows][row_len] float32 images        d_labels  [n_rows] int64 class indices
 *   d_perm    [n_rows] int32: row b's partner         d_coef    [n_rows][2] float32 (a_b, c_b) = (lam, 1 - lam), each
 *                                                               formed in float64 and rounded to float by the caller
 *   d_out     [n_rows][row_len]:  out[b]  = a_b x[b] + c_b x[perm[b]]           (must not alias d_x)
 *   d_soft    [n_rows][2]:        soft[b] = a_b onehot(y[b]) + c_b onehot(y[perm[b]])
 * Each product is rounded on its own (torch's `lam * x1 + (1 - lam) * x2`, no fused multiply-add): cough_mix_rows'
 * arithmetic, so both outputs equal its results bit for bit.  A label outside {0, 1} has the all-zero one-hot.  The
 * host cannot check a permutation that lives on the device: an entry outside 0..n_rows-1 means "no partner", and the row
 * comes back as it is (out[b] = x[b], soft[b] = onehot(y[b])).  n_rows >= 1, row_len >= 1. */
int cough_mix_batch(const float* d_x, const long long* d_labels, const int* d_perm, const float* d_coef, int n_rows,
                    long long row_len, float* d_out, float* d_soft, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_SOFT_H */
