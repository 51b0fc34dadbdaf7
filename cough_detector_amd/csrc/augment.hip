// Waveform augmentation and MixUp: the batched counterpart of AudioAugmentor.augment and MixUp.__call__
// (/root/reference/src/augmentation.py:249-268, :353-369).  Training-side, memory-bound: one workgroup per clip applies
// the clip's whole chain (shift -> gain -> gaussian noise at a drawn SNR -> bank noise at a drawn SNR), each noise step
// behind a per-clip power reduction.  A clip of up to AUG_LDS_MAX samples is staged in LDS and read from HBM once;
// longer clips take the same passes over global memory, recomputing the shifted, scaled clip from the input and keeping
// an intermediate only in the output row.  All reductions are fp32 in a fixed order (per-thread strided sums, DPP wave
// sums, waves summed in index order), so a result is the same from run to run.
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"
#include "philox.h"

namespace cough {
namespace {

#include "augment_kernel.h"

// MixUp: out[row] = a[row] * x1[row] + c[row] * x2[idx[row]] with (a, c) = (lam, 1 - lam) rounded to float by the
// caller, each product rounded on its own (torch's `lam * x1 + (1 - lam) * x2`, no fused multiply-add).
__global__ __launch_bounds__(256) void mix_rows_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                       const int* __restrict__ idx, float* __restrict__ out,
                                                       long long n_rows, long long row_len, const float2* __restrict__ coef) {
    const long long row = blockIdx.y + (long long)blockIdx.z * 65535;
    if (row >= n_rows) return;
    const float2 ac = coef[row];
    long long src = row;
    if (idx) {
        src = idx[row];
        if (src < 0 || src >= n_rows) src = -1;   // checked by the caller; never read outside x2
    }
    const float* a = x1 + row * row_len;
    float* d = out + row * row_len;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < row_len; i += (long long)gridDim.x * blockDim.x) {
        if (src < 0) { d[i] = __int_as_float(0x7fc00000); continue; }
        d[i] = mul_rn(ac.x, a[i]) + mul_rn(ac.y, x2[src * row_len + i]);
    }
}

}  // namespace
}  // namespace cough

extern "C" size_t cough_augment_workspace_bytes(int n_clips) {
    if (n_clips <= 0) return 0;
    return (size_t(n_clips) * sizeof(cough::AugRec) + 255) / 256 * 256;
}

extern "C" int cough_augment_waveforms(const float* d_in, long long in_stride, float* d_out, int n_clips, int n_samples,
                                       const int* lengths, const cough_aug_clip* clips, const float* d_bank,
                                       long long bank_numel, const long long* bank_offsets, const int* bank_lengths,
                                       int n_bank, const float* d_gaussian, unsigned long long seed, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(n_clips >= 0 && n_samples >= 1 && in_stride >= n_samples && n_bank >= 0 && bank_numel >= 0, COUGH_EINVAL,
                  "cough_augment_waveforms: bad sizes (%d clips of %d samples, stride %lld, %d bank entries, %lld bank samples)",
                  n_clips, n_samples, in_stride, n_bank, bank_numel);
    if (n_clips == 0) return COUGH_OK;
    COUGH_REQUIRE(d_in && d_out && clips && d_workspace, COUGH_EINVAL, "cough_augment_waveforms: NULL argument");
    COUGH_REQUIRE(d_out != d_in, COUGH_EINVAL, "cough_augment_waveforms: d_out must not alias d_in");
    COUGH_REQUIRE(workspace_bytes >= cough_augment_workspace_bytes(n_clips) && (reinterpret_cast<uintptr_t>(d_workspace) & 255) == 0,
                  COUGH_EWORKSPACE, "cough_augment_waveforms: workspace of %zu bytes (need %zu, 256-byte aligned)", workspace_bytes,
                  cough_augment_workspace_bytes(n_clips));
    if (n_bank > 0) {
        COUGH_REQUIRE(d_bank && bank_offsets && bank_lengths, COUGH_EINVAL, "cough_augment_waveforms: NULL noise-bank argument");
        for (int k = 0; k < n_bank; ++k)
            COUGH_REQUIRE(bank_lengths[k] >= 1 && bank_offsets[k] >= 0 && bank_offsets[k] + bank_lengths[k] <= bank_numel,
                          COUGH_EINVAL, "cough_augment_waveforms: bank entry %d (offset %lld, length %d) outside the %lld-sample bank",
                          k, bank_offsets[k], bank_lengths[k], bank_numel);
    }
    std::vector<AugRec> recs(n_clips);
    for (int b = 0; b < n_clips; ++b) {
        const cough_aug_clip& c = clips[b];
        const int L = lengths ? lengths[b] : n_samples;
        COUGH_REQUIRE(L >= 1 && L <= n_samples, COUGH_EINVAL, "cough_augment_waveforms: lengths[%d] = %d (1..%d)", b, L, n_samples);
        COUGH_REQUIRE(c.shift > -L && c.shift < L, COUGH_EINVAL, "cough_augment_waveforms: clip %d: shift %d for a length of %d",
                      b, c.shift, L);
        COUGH_REQUIRE(c.gaussian == 0 || c.gaussian == 1, COUGH_EINVAL, "cough_augment_waveforms: clip %d: gaussian = %d (0 / 1)", b,
                      c.gaussian);
        COUGH_REQUIRE(c.bank_index >= -1 && c.bank_index < n_bank, COUGH_EINVAL,
                      "cough_augment_waveforms: clip %d: bank_index %d (-1 or 0..%d)", b, c.bank_index, n_bank - 1);
        AugRec& r = recs[b];
        r = AugRec{};
        r.len = L;
        r.shift = c.shift;
        r.gain = c.gain;
        r.gauss = c.gaussian;
        r.gauss_snr = float(std::pow(10.0, c.gaussian_snr_db / 10.0));
        if (c.bank_index >= 0) {
            const long long bl = bank_lengths[c.bank_index];
            // the reference repeats a shorter entry to (L / bl + 1) * bl samples and crops L of them from `start` (:140-151)
            const long long rep = bl < L ? (L / bl + 1) * bl : bl;
            COUGH_REQUIRE(c.bank_start >= 0 && c.bank_start <= rep - L, COUGH_EINVAL,
                          "cough_augment_waveforms: clip %d: bank_start %lld (0..%lld)", b, c.bank_start, rep - L);
            r.bank = 1;
            r.bank_off = bank_offsets[c.bank_index];
            r.bank_len = unsigned(bl);
            r.bank_start = unsigned(c.bank_start % bl);
            r.bank_snr = float(std::pow(10.0, c.bank_snr_db / 10.0));
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    COUGH_HIP_CHECK(hipMemcpyAsync(d_workspace, recs.data(), recs.size() * sizeof(AugRec), hipMemcpyHostToDevice, st));
    const AugRec* d_recs = static_cast<const AugRec*>(d_workspace);
    if (n_samples <= AUG_LDS_MAX)
        hipLaunchKernelGGL(augment_kernel<true>, dim3(n_clips), dim3(AUG_THREADS), size_t((n_samples + 3) / 4) * 16, st, d_in,
                           in_stride, d_out, n_samples, d_recs, d_bank, d_gaussian, seed, nullptr);
    else
        hipLaunchKernelGGL(augment_kernel<false>, dim3(n_clips), dim3(AUG_THREADS), 0, st, d_in, in_stride, d_out, n_samples,
                           d_recs, d_bank, d_gaussian, seed, nullptr);
    COUGH_HIP_CHECK(hipGetLastError());
    // a copy from pageable host memory is performed synchronously (hip_runtime_api.h, hipMemcpyAsync): `recs` may go out of scope
    return COUGH_OK;
}

extern "C" int cough_mix_rows(const float* d_x1, const float* d_x2, const int* d_index2, float* d_out, long long n_rows,
                              long long row_len, const float* d_coef, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(n_rows >= 0 && row_len >= 0 && n_rows <= 65535LL * 65535LL, COUGH_EINVAL,
                  "cough_mix_rows: bad sizes (%lld rows of %lld)", n_rows, row_len);
    if (n_rows == 0 || row_len == 0) return COUGH_OK;
    COUGH_REQUIRE(d_x1 && d_x2 && d_out && d_coef, COUGH_EINVAL, "cough_mix_rows: NULL argument");
    const long long per_row = (row_len + 255) / 256;
    const unsigned gx = unsigned(per_row < 64 ? per_row : 64);
    const unsigned gy = unsigned(n_rows < 65535 ? n_rows : 65535), gz = unsigned((n_rows + 65534) / 65535);
    hipLaunchKernelGGL(mix_rows_kernel, dim3(gx, gy, gz), dim3(256), 0, static_cast<hipStream_t>(stream), d_x1, d_x2, d_index2,
                       d_out, n_rows, row_len, reinterpret_cast<const float2*>(d_coef));
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
