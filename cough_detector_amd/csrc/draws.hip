// libcough_amd_draws.so: a training batch's random draws on the device (include/cough_amd_draws.h).  The draw kernel writes
// one cough_aug_clip and the SpecAugment mask triples per row from a seeded Philox stream; the resolve kernel turns device
// records into the augment kernel's AugRec (making a record it cannot use harmless), and augment_kernel.h's kernel -- the
// one libcough_amd.so runs -- then reads each row in place from the packed bank.
//
// Access width.  A row of the bank starts at any element, so the augment kernel reads x[j] as 4-byte scalars (a wave's 64
// consecutive floats still coalesce into whole cache lines); what it writes is a matrix row.  The draw and resolve kernels
// move 40 to 48 bytes per thread: launch-bound, not bandwidth-bound.
#include "../../include/cough_amd_draws.h"

#include <cstdint>
#include <cstring>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

#include "augment_kernel.h"

constexpr int DT = 64;         // threads of the draw and resolve kernels: one row each

struct DrawArgs {
    unsigned long long seed;
    int n_rows;
    int aug, spec;             // which of the two is switched on
    double p_augment, spec_p;
    int n_bank;
    int n_freq, freq_param, n_time, time_param, height, width;
};

// The reference repeats a shorter entry to (n / bl + 1) * bl samples before it crops n of them (augmentation.py:140-151).
__device__ __forceinline__ long long repeated_length(long long bl, long long n) { return bl < n ? (n / bl + 1) * bl : bl; }

// ------------------------------------------------------------------------------------------ the draws of one row
// The contract of cough_amd_draws.h, operator by operator.  tests/draws_ref.py restates it in numpy, which has no fused
// multiply-add, and the records are compared bit for bit: contraction is off for this function (hipcc's default is
// -ffp-contract=fast, and its __dmul_rn / __dadd_rn are the plain operators).
__global__ __launch_bounds__(DT) void draw_kernel(DrawArgs a, const int* __restrict__ lengths,
                                                  const int* __restrict__ bank_lengths, cough_aug_clip* __restrict__ clips,
                                                  int* __restrict__ m_axis, int* __restrict__ m_start, int* __restrict__ m_end) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= a.n_rows) return;
    const uint2 key = make_uint2(unsigned(a.seed), unsigned(a.seed >> 32));
    auto slot = [&](unsigned s) { return philox4x32_10(make_uint4(s, unsigned(row), 0u, 1u), key); };
    auto unit = [](unsigned x) { return (double(x) + 0.5) * 0x1p-32; };       // exact; strictly inside (0, 1)
    const uint4 s2 = slot(2u);
    if (a.aug) {
        cough_aug_clip c;
        c.shift = 0;
        c.gain = 1.0f;
        c.gaussian = 0;
        c.bank_index = -1;
        c.gaussian_snr_db = 0.0;
        c.bank_snr_db = 0.0;
        c.bank_start = 0;
        const int n = lengths[row];
        if (n >= 1) {
            const uint4 s0 = slot(0u), s1 = slot(1u);
            if (unit(s0.x) <= a.p_augment) {
                const double f = -0.2 + 0.4 * unit(s0.y);
                c.shift = int(double(n) * f);
            }
            if (unit(s0.z) <= a.p_augment) c.gain = float(0.7 + 0.6 * unit(s0.w));
            if (unit(s1.x) <= a.p_augment) {
                c.gaussian = 1;
                c.gaussian_snr_db = 10.0 + 20.0 * unit(s1.y);
            }
            if (unit(s1.z) <= a.p_augment && a.n_bank > 0) {
                int k = int(unit(s2.x) * double(a.n_bank));
                k = k < a.n_bank - 1 ? k : a.n_bank - 1;
                const long long bl = bank_lengths[k];
                if (bl >= 1) {
                    const long long rep = repeated_length(bl, n);
                    long long start = (long long)(unit(s2.y) * double(rep - n + 1));
                    start = start < rep - n ? start : rep - n;
                    c.bank_index = k;
                    c.bank_start = start;
                    c.bank_snr_db = 5.0 + 15.0 * unit(s1.w);
                }
            }
        }
        clips[row] = c;
    }
    if (a.spec) {
        const bool fired = unit(s2.w) <= a.spec_p;
        const int n_masks = a.n_freq + a.n_time;
        for (int m = 0; m < n_masks; ++m) {
            int axis = 0, start = 0, end = 0;
            if (fired) {
                const uint4 s = slot(3u + unsigned(m));
                axis = m < a.n_freq ? 0 : 1;
                const double param = double(axis == 0 ? a.freq_param : a.time_param);
                const double size = double(axis == 0 ? a.height : a.width);
                const double value = unit(s.x) * param;
                const double minv = unit(s.y) * (size - value);
                start = int(minv);
                end = start + int(value);
            }
            const long long j = (long long)row * n_masks + m;
            m_axis[j] = axis;
            m_start[j] = start;
            m_end[j] = end;
        }
    }
}

// ------------------------------------------------------------------------------------------ device records -> AugRec
// What cough_augment_waveforms does on the host after its checks; here a record that would fail a check is made harmless
// (cough_amd_draws.h lists how).
__global__ __launch_bounds__(DT) void resolve_kernel(const cough_aug_clip* __restrict__ clips, const int* __restrict__ lengths,
                                                     int n_rows, int n_samples, const long long* __restrict__ bank_offsets,
                                                     const int* __restrict__ bank_lengths, int n_bank, long long bank_numel,
                                                     AugRec* __restrict__ recs) {
    const int b = blockIdx.x * DT + threadIdx.x;
    if (b >= n_rows) return;
    const cough_aug_clip c = clips[b];
    const int L = min(max(lengths[b], 0), n_samples);
    AugRec r{};
    r.len = L;
    r.shift = min(max(c.shift, -L), L);        // |shift| >= L: every sample is shifted out, whatever the value
    r.gain = c.gain;
    r.gauss = (c.gaussian == 1 && L >= 1) ? 1 : 0;
    r.gauss_snr = float(pow(10.0, c.gaussian_snr_db / 10.0));
    if (L >= 1 && c.bank_index >= 0 && c.bank_index < n_bank) {
        const long long bl = bank_lengths[c.bank_index], off = bank_offsets[c.bank_index];
        if (bl >= 1 && off >= 0 && off <= bank_numel - bl) {
            const long long rep = repeated_length(bl, L);
            if (c.bank_start >= 0 && c.bank_start <= rep - L) {
                r.bank = 1;
                r.bank_off = off;
                r.bank_len = unsigned(bl);
                r.bank_start = unsigned(c.bank_start % bl);
                r.bank_snr = float(pow(10.0, c.bank_snr_db / 10.0));
            }
        }
    }
    recs[b] = r;
}

}  // namespace
}  // namespace cough

extern "C" int cough_draws_abi_version(void) { return COUGH_DRAWS_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_draws_last_error)

extern "C" int cough_draw_batch(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int n_bank,
                                const int* d_bank_lengths, double spec_p, int n_freq_masks, int freq_mask_param,
                                int n_time_masks, int time_mask_param, int height, int width, cough_aug_clip* d_clips_out,
                                int* d_mask_axis, int* d_mask_start, int* d_mask_end, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_batch";
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(n_bank >= 0, COUGH_EINVAL, "%s: n_bank must not be negative, got %d", fn, n_bank);
    COUGH_REQUIRE(p_augment == p_augment && spec_p == spec_p, COUGH_EINVAL, "%s: a probability is NaN (p_augment %g, spec_p %g)",
                  fn, p_augment, spec_p);
    COUGH_REQUIRE(n_freq_masks >= 0 && n_time_masks >= 0 && n_freq_masks <= COUGH_MAX_MASKS && n_time_masks <= COUGH_MAX_MASKS &&
                      n_freq_masks + n_time_masks <= COUGH_MAX_MASKS,
                  COUGH_EINVAL, "%s: n_masks = %d + %d (0..%d in all)", fn, n_freq_masks, n_time_masks, COUGH_MAX_MASKS);
    const bool aug = p_augment >= 0.0, spec = spec_p >= 0.0 && n_freq_masks + n_time_masks > 0;
    if (spec) {
        COUGH_REQUIRE(height >= 1 && width >= 1, COUGH_EINVAL, "%s: bad shape (%d x %d)", fn, height, width);
        COUGH_REQUIRE(n_freq_masks == 0 || (freq_mask_param >= 1 && freq_mask_param <= height), COUGH_EINVAL,
                      "%s: freq_mask_param = %d (1..%d, the height)", fn, freq_mask_param, height);
        COUGH_REQUIRE(n_time_masks == 0 || (time_mask_param >= 1 && time_mask_param <= width), COUGH_EINVAL,
                      "%s: time_mask_param = %d (1..%d, the width)", fn, time_mask_param, width);
        COUGH_REQUIRE(d_mask_axis && d_mask_start && d_mask_end, COUGH_EINVAL, "%s: NULL mask array", fn);
        COUGH_REQUIRE(aligned(d_mask_axis, 4) && aligned(d_mask_start, 4) && aligned(d_mask_end, 4), COUGH_EINVAL,
                      "%s: int32 arrays must be 4-byte aligned", fn);
    }
    if (aug) {
        COUGH_REQUIRE(d_lengths && d_clips_out && (n_bank == 0 || d_bank_lengths), COUGH_EINVAL, "%s: NULL argument", fn);
        COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_bank_lengths, 4), COUGH_EINVAL,
                      "%s: int32 arrays must be 4-byte aligned", fn);
        COUGH_REQUIRE(aligned(d_clips_out, 8), COUGH_EINVAL, "%s: d_clips_out must be 8-byte aligned", fn);
    }
    if (n_rows == 0 || !(aug || spec)) return COUGH_OK;
    DrawArgs a{};
    a.seed = seed;
    a.n_rows = n_rows;
    a.aug = aug;
    a.spec = spec;
    a.p_augment = p_augment;
    a.spec_p = spec_p;
    a.n_bank = n_bank;
    a.n_freq = n_freq_masks;
    a.freq_param = freq_mask_param;
    a.n_time = n_time_masks;
    a.time_param = time_mask_param;
    a.height = height;
    a.width = width;
    hipLaunchKernelGGL(draw_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream), a,
                       d_lengths, d_bank_lengths, d_clips_out, d_mask_axis, d_mask_start, d_mask_end);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" size_t cough_augment_rows_drawn_workspace_bytes(int n_rows) {
    if (n_rows <= 0) return 0;
    return (size_t(n_rows) * sizeof(cough::AugRec) + 255) / 256 * 256;
}

extern "C" int cough_augment_rows_drawn(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                        int n_samples, const cough_aug_clip* d_clips, const float* d_bank, long long bank_numel,
                                        const long long* d_bank_offsets, const int* d_bank_lengths, int n_bank,
                                        unsigned long long seed, float* d_out, void* d_workspace, size_t workspace_bytes,
                                        void* stream) {
    using namespace cough;
    const char* fn = "cough_augment_rows_drawn";
    COUGH_REQUIRE(n_rows >= 0 && n_samples >= 1 && n_bank >= 0 && bank_numel >= 0, COUGH_EINVAL,
                  "%s: bad sizes (%d rows of %d samples, %d bank entries, %lld bank samples)", fn, n_rows, n_samples, n_bank,
                  bank_numel);
    COUGH_REQUIRE(n_samples <= (1 << 30), COUGH_EUNSUPPORTED, "%s: n_samples = %d is more than 2^30", fn, n_samples);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_clips && d_out && d_workspace, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_bank == 0 || (d_bank && d_bank_offsets && d_bank_lengths), COUGH_EINVAL, "%s: NULL noise-bank argument", fn);
    COUGH_REQUIRE(d_out != d_src, COUGH_EINVAL, "%s: d_out must not alias d_src", fn);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4) && aligned(d_bank, 4) && aligned(d_bank_lengths, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8) && aligned(d_clips, 8) && aligned(d_bank_offsets, 8), COUGH_EINVAL,
                  "%s: d_row_offsets, d_clips and d_bank_offsets must be 8-byte aligned", fn);
    COUGH_REQUIRE(workspace_bytes >= cough_augment_rows_drawn_workspace_bytes(n_rows) && aligned(d_workspace, 256),
                  COUGH_EWORKSPACE, "%s: workspace of %zu bytes (need %zu, 256-byte aligned)", fn, workspace_bytes,
                  cough_augment_rows_drawn_workspace_bytes(n_rows));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    AugRec* d_recs = static_cast<AugRec*>(d_workspace);
    hipLaunchKernelGGL(resolve_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, st, d_clips, d_lengths, n_rows,
                       n_samples, d_bank_offsets, d_bank_lengths, n_bank, bank_numel, d_recs);
    COUGH_HIP_CHECK(hipGetLastError());
    const float* no_gaussian = nullptr;        // the noise is always the seeded generator's
    if (n_samples <= AUG_LDS_MAX)
        hipLaunchKernelGGL(augment_kernel<true>, dim3(n_rows), dim3(AUG_THREADS), size_t((n_samples + 3) / 4) * 16, st, d_src, 0LL,
                           d_out, n_samples, d_recs, d_bank, no_gaussian, seed, d_row_offsets);
    else
        hipLaunchKernelGGL(augment_kernel<false>, dim3(n_rows), dim3(AUG_THREADS), 0, st, d_src, 0LL, d_out, n_samples, d_recs,
                           d_bank, no_gaussian, seed, d_row_offsets);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
