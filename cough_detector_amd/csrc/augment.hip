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

constexpr int AUG_THREADS = 512;
constexpr int AUG_WAVES = AUG_THREADS / 64;
constexpr int AUG_LDS_MAX = 16256;   // floats: 65 024 B of dynamic LDS (a 1 s clip at 16 kHz), plus the reduction slots

// The per-clip record the kernel reads, resolved on the host from cough_aug_clip after every check has passed.
struct AugRec {
    long long bank_off;   // first sample of the bank entry in d_bank
    int len;              // samples of the clip (<= n_samples); the tail [len, n_samples) is written as 0
    int shift;            // y[i] = x[i - shift] inside [0, len)
    float gain;
    int gauss;            // 1: add_gaussian_noise fired
    float gauss_snr;      // 10^(snr_db / 10)
    int bank;             // 1: add_noise fired
    float bank_snr;
    unsigned bank_len;
    unsigned bank_start;  // crop start reduced modulo bank_len: sample i of the crop is entry[(bank_start + i) % bank_len]
    int pad;
};

// Four standard normals for samples 4g .. 4g+3 of clip b (two Box-Muller pairs, 24-bit uniforms, u1 in (0, 1]).
__device__ __forceinline__ float4 gauss4(unsigned long long seed, int b, int g) {
    const uint4 r = philox4x32_10(make_uint4(unsigned(g), unsigned(b), 0u, 0u),
                                  make_uint2(unsigned(seed), unsigned(seed >> 32)));
    const float s24 = 1.0f / 16777216.0f;
    const float ra = sqrtf(-2.0f * logf(float((r.x >> 8) + 1u) * s24));
    const float rb = sqrtf(-2.0f * logf(float((r.z >> 8) + 1u) * s24));
    float sa, ca, sb, cb;
    sincospif(2.0f * float(r.y >> 8) * s24, &sa, &ca);
    sincospif(2.0f * float(r.w >> 8) * s24, &sb, &cb);
    return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

// Sum over the workgroup in a fixed order; every thread gets the total.  `red` holds AUG_WAVES slots.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                       // the previous reduction's readers are done with `red`
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < AUG_WAVES; ++w) s += red[w];
    return s;
}

// One workgroup per clip.  STAGED: the shifted, scaled clip (and later the clip after the gaussian step) lives in LDS;
// otherwise it is recomputed from the input, and the clip after the gaussian step is kept in the output row.  The passes
// that touch that intermediate use the sample-group mapping (thread t: samples 4g .. 4g+3, g = t + k * AUG_THREADS),
// so every thread reads back only what it wrote.
template <bool STAGED>
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const float* __restrict__ in, long long in_stride,
                                                              float* __restrict__ out, int n, const AugRec* __restrict__ recs,
                                                              const float* __restrict__ bank, const float* __restrict__ zbuf,
                                                              unsigned long long seed) {
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    __shared__ float red[AUG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const AugRec r = recs[b];
    const float* x = in + (long long)b * in_stride;
    float* o = out + (long long)b * n;
    const float* z = zbuf ? zbuf + (long long)b * n : nullptr;
    const float* nb = bank + r.bank_off;
    const int L = r.len;
    const float fl = float(L);           // torch's mean: the sum divided by the count

    auto clean = [&](int i) {              // time_shift + volume_perturbation (speed_perturbation is the identity)
        const int j = i - r.shift;
        return (j >= 0 && j < L) ? x[j] * r.gain : 0.0f;
    };
    auto bank_at = [&](int i) {
        unsigned j = r.bank_start + unsigned(i);
        if (j >= r.bank_len) j %= r.bank_len;
        return nb[j];
    };
    auto z4 = [&](int g) {                 // the gaussian noise of samples 4g .. 4g+3 (entries past the clip: unused)
        if (!z) return gauss4(seed, b, g);
        const int i = 4 * g;
        return make_float4(z[i], i + 1 < L ? z[i + 1] : 0.f, i + 2 < L ? z[i + 2] : 0.f, i + 3 < L ? z[i + 3] : 0.f);
    };

    if (!r.gauss && !r.bank) {             // no noise step: one pass, no reduction
        for (int i = tid; i < n; i += AUG_THREADS) o[i] = i < L ? clean(i) : 0.0f;
        return;
    }

    // pass 1: P = mean(y^2) of the shifted, scaled clip
    float acc = 0.f;
    for (int i = tid; i < L; i += AUG_THREADS) {
        const float v = clean(i);
        if (STAGED) lds[i] = v;
        acc += v * v;
    }
    float power = block_sum(acc, red) / fl;
    bool in_buf = STAGED;                  // the current clip is in lds (STAGED) / in o (otherwise); else recompute
    auto cur = [&](int i) { return in_buf ? (STAGED ? lds[i] : o[i]) : clean(i); };
    const int groups = (L + 3) >> 2;

    float gscale = 0.f;
    bool gauss_pending = false;
    if (r.gauss) {
        // add_gaussian_noise: Pz = mean(z^2) of the noise actually drawn
        acc = 0.f;
        for (int g = tid; g < groups; g += AUG_THREADS) {
            const float4 v = z4(g);
            const int i = 4 * g;
            acc += v.x * v.x;
            if (i + 1 < L) acc += v.y * v.y;
            if (i + 2 < L) acc += v.z * v.z;
            if (i + 3 < L) acc += v.w * v.w;
        }
        const float pz = block_sum(acc, red) / fl;
        gscale = sqrtf(power / (r.gauss_snr * pz));
        gauss_pending = true;
        if (r.bank) {                      // add_noise reduces over the result: materialise it and take its power
            acc = 0.f;
            for (int g = tid; g < groups; g += AUG_THREADS) {
                const float4 v = z4(g);
                const float zz[4] = {v.x, v.y, v.z, v.w};
                for (int k = 0; k < 4; ++k) {
                    const int i = 4 * g + k;
                    if (i < L) {
                        const float y = cur(i) + gscale * zz[k];
                        if (STAGED) lds[i] = y; else o[i] = y;
                        acc += y * y;
                    }
                }
            }
            in_buf = true;
            gauss_pending = false;
            power = block_sum(acc, red) / fl;
        }
    }

    float bscale = 0.f;
    bool bank_on = false;
    if (r.bank) {
        // add_noise: the crop's power; nothing is added when it is not > 0 (augmentation.py:158)
        acc = 0.f;
        for (int i = tid; i < L; i += AUG_THREADS) {
            const float v = bank_at(i);
            acc += v * v;
        }
        const float pn = block_sum(acc, red) / fl;
        if (pn > 0.f) {
            bscale = sqrtf(power / (r.bank_snr * pn));
            bank_on = true;
        }
    }

    // final pass: out = clip (+ gaussian) (+ bank crop), tail zero
    for (int g = tid; 4 * g < n; g += AUG_THREADS) {
        float zz[4] = {0.f, 0.f, 0.f, 0.f};
        if (gauss_pending && 4 * g < L) {
            const float4 v = z4(g);
            zz[0] = v.x; zz[1] = v.y; zz[2] = v.z; zz[3] = v.w;
        }
        for (int k = 0; k < 4; ++k) {
            const int i = 4 * g + k;
            if (i >= n) break;
            float y = 0.f;
            if (i < L) {
                y = cur(i);
                if (gauss_pending) y = y + gscale * zz[k];
                if (bank_on) y = y + bscale * bank_at(i);
            }
            o[i] = y;
        }
    }
}

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
                           in_stride, d_out, n_samples, d_recs, d_bank, d_gaussian, seed);
    else
        hipLaunchKernelGGL(augment_kernel<false>, dim3(n_clips), dim3(AUG_THREADS), 0, st, d_in, in_stride, d_out, n_samples,
                           d_recs, d_bank, d_gaussian, seed);
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
