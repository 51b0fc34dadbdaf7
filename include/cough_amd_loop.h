/*
 * cough_amd_loop.h -- C-ABI of libcough_amd_loop.so, the companion of libcough_amd.so for the epoch loop around the
 * training step (the reference's src/train.py outside train_epoch's step: validate :114-180, the running metrics of
 * train_epoch :97-100).
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points, so what the loop needs on the device is exported from a
 * library of its own with a version of its own.  The conventions are those of cough_amd.h: plain pointers and sizes
 * only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a
 * thread-local message for the last-error call below; launches are stream-ordered on `stream` (a hipStream_t; NULL =
 * default stream); no call allocates or synchronises; every argument is checked before the launch.
 */
#ifndef COUGH_AMD_LOOP_H
#define COUGH_AMD_LOOP_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_loop_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_LOOP_ABI_VERSION 1

int cough_loop_abi_version(void);
const char* cough_loop_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ epoch meter
 * The running metrics of an epoch, kept on the device so that the host reads them once, at the end of the epoch:
 * src/train.py:97-100 (train_epoch: running_loss += loss.item(), outputs.max(1), total, correct) and :149-155, :161-164
 * (validate: the same, plus the confusion counts of the cough class).  64 bytes of device memory, zeroed by the caller
 * with a stream-ordered memset before the first update of an epoch. */
typedef struct cough_epoch_meter {
    double loss_sum;      /* sum over the batches of the batch loss, each rounded to float32 first (loss.item()) */
    long long n_batches;  /* updates since the memset */
    long long total;      /* clips seen */
    long long correct;    /* clips whose prediction equals the target */
    long long tp, fp, fn, tn; /* (pred, target) = (1, 1), (1, 0), (0, 1), (0, 0) */
} cough_epoch_meter;
#define COUGH_EPOCH_METER_BYTES 64

/* One batch into the meter: one launch of one workgroup; updates of one meter are ordered by the stream, so nothing is
 * atomic and the same batches in the same order give the same bits.
 *   d_logits [n_clips][2] float32, d_targets [n_clips] int64, n_clips >= 1
 *   d_class_weights [2] float32 or NULL: CrossEntropyLoss(weight=...)
 *   d_batch_loss [1] float32 or NULL.  NULL: the batch loss is computed here, sum of w_y (logsumexp(z) - z_y) over
 *       sum of w_y, the per-clip terms in float32 as the training steps form them, the sums in double in a fixed order
 *       (thread t takes clips t, t + 256, ... in order, then a fixed pairwise tree), the quotient rounded to float32.
 *       Non-NULL: that value (a training step's d_loss) is taken instead and no loss is computed.
 *       Either way the float32 is added to loss_sum as a double.  A NaN logit or a target outside {0, 1} makes the
 *       computed loss NaN.
 *   prediction, as torch's outputs.max(1): class 1 iff z1 > z0, or z1 is NaN and z0 is not
 *   counts: total += n_clips; a target outside {0, 1} enters no other count
 *   d_preds [n_clips] int64 or NULL: receives the predictions
 * d_targets, d_meter and d_preds must be 8-byte aligned, the float32 arrays 4-byte aligned. */
int cough_epoch_meter_update(const float* d_logits, const long long* d_targets, int n_clips,
                             const float* d_class_weights, const float* d_batch_loss, cough_epoch_meter* d_meter,
                             long long* d_preds, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_LOOP_H */
