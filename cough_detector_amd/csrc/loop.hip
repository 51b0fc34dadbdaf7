// libcough_amd_loop.so: the device side of the epoch loop (include/cough_amd_loop.h).  One kernel: the epoch meter, which
// keeps the running loss and the prediction counts of the reference's train_epoch / validate (src/train.py:97-100,
// :149-155, :161-164) in device memory, so that an epoch reads them back once.
#include "../../include/cough_amd_loop.h"
#include "train_common.h"

namespace cough {

namespace {

static_assert(sizeof(cough_epoch_meter) == COUGH_EPOCH_METER_BYTES, "cough_epoch_meter is 64 bytes");

// torch's outputs.max(1) on two columns: the first NaN wins, otherwise the first of the largest
__device__ __forceinline__ int predict2(float z0, float z1) {
    return (z1 > z0 || (z1 != z1 && z0 == z0)) ? 1 : 0;
}

// one workgroup: thread t takes clips t, t + 256, ... in order, then a fixed pairwise tree over the threads
__global__ __launch_bounds__(NT) void epoch_meter_kernel(const float* __restrict__ logits,
                                                         const long long* __restrict__ targets, int B,
                                                         const float* __restrict__ class_w,
                                                         const float* __restrict__ batch_loss,
                                                         cough_epoch_meter* __restrict__ meter,
                                                         long long* __restrict__ preds) {
    __shared__ double sh[2][NT];
    __shared__ int cnt[5][NT];
    const int t = threadIdx.x;
    double s = 0.0, w = 0.0;
    int correct = 0, tp = 0, fp = 0, fn = 0, tn = 0;
    for (int b = t; b < B; b += NT) {
        const float z0 = logits[2 * (long long)b], z1 = logits[2 * (long long)b + 1];
        const long long y = targets[b];
        const int pred = predict2(z0, z1);
        if (preds) preds[b] = pred;
        if (y == 0 || y == 1) {
            correct += pred == int(y);
            tp += pred & int(y);
            fp += pred & (1 - int(y));
            fn += (1 - pred) & int(y);
            tn += (1 - pred) & (1 - int(y));
        }
        if (!batch_loss) {
            float lg[2], wn[2];
            ce_terms(0, z0, z1, targets + b, nullptr, class_w, lg, wn);
            s += double(wn[0]);
            w += double(wn[1]);
        }
    }
    sh[0][t] = s; sh[1][t] = w;
    cnt[0][t] = correct; cnt[1][t] = tp; cnt[2][t] = fp; cnt[3][t] = fn; cnt[4][t] = tn;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) {
            sh[0][t] += sh[0][t + off];
            sh[1][t] += sh[1][t + off];
#pragma unroll
            for (int k = 0; k < 5; ++k) cnt[k][t] += cnt[k][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float loss = batch_loss ? batch_loss[0] : float(sh[0][0] / sh[1][0]);
        meter->loss_sum += double(loss);
        meter->n_batches += 1;
        meter->total += B;
        meter->correct += cnt[0][0];
        meter->tp += cnt[1][0];
        meter->fp += cnt[2][0];
        meter->fn += cnt[3][0];
        meter->tn += cnt[4][0];
    }
}

}  // namespace
}  // namespace cough

extern "C" int cough_loop_abi_version(void) { return COUGH_LOOP_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_loop_last_error)

extern "C" int cough_epoch_meter_update(const float* d_logits, const long long* d_targets, int n_clips,
                                        const float* d_class_weights, const float* d_batch_loss,
                                        cough_epoch_meter* d_meter, long long* d_preds, void* stream) {
    using namespace cough;
    const char* fn = "cough_epoch_meter_update";
    COUGH_REQUIRE(d_logits && d_targets && d_meter, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips > 0, COUGH_EINVAL, "%s: n_clips must be positive, got %d", fn, n_clips);
    COUGH_REQUIRE(aligned(d_logits, 4) && aligned(d_class_weights, 4) && aligned(d_batch_loss, 4), COUGH_EINVAL,
                  "%s: float32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_targets, 8) && aligned(d_meter, 8) && aligned(d_preds, 8), COUGH_EINVAL,
                  "%s: d_targets, d_meter and d_preds must be 8-byte aligned", fn);
    hipLaunchKernelGGL(epoch_meter_kernel, dim3(1), dim3(NT), 0, static_cast<hipStream_t>(stream), d_logits, d_targets,
                       n_clips, d_class_weights, d_batch_loss, d_meter, d_preds);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
