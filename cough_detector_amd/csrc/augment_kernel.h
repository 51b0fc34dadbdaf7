// The waveform-augmentation kernel, shared by augment.hip (libcough_amd.so: records resolved on the host, rows of a
// matrix) and draws.hip (libcough_amd_draws.so: records resolved on the device, rows read in place from a packed bank), so
// that both libraries run one kernel.  Include it inside `namespace cough { namespace { ... } }`, after common.h and
// philox.h.
#pragma once

constexpr int AUG_THREADS = 512;
constexpr int AUG_WAVES = AUG_THREADS / 64;
constexpr int AUG_LDS_MAX = 16256;   // floats: 65 024 B of dynamic LDS (a 1 s clip at 16 kHz), plus the reduction slots

// The per-clip record the kernel reads, resolved from cough_aug_clip: on the host after every check has passed, or by
// draws.hip's resolve kernel, which makes a record it cannot use harmless.
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
// so every thread reads back only what it wrote.  Clip b is read at in + row_offsets[b], or at in + b * in_stride when
// row_offsets is null; a row may start at any element, so x[j] is read as scalars.
template <bool STAGED>
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const float* __restrict__ in, long long in_stride,
                                                              float* __restrict__ out, int n, const AugRec* __restrict__ recs,
                                                              const float* __restrict__ bank, const float* __restrict__ zbuf,
                                                              unsigned long long seed, const long long* __restrict__ row_offsets) {
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    __shared__ float red[AUG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const AugRec r = recs[b];
    const float* x = in + (row_offsets ? row_offsets[b] : (long long)b * in_stride);
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
