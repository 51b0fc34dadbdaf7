// libcough_amd_channel.so: the capture channel on the device (include/cough_amd_channel.h).  Every row of a batch goes
// through a cascade of second-order IIR sections out of a prepared bank -- the microphone's response -- and a hard
// clip relative to its own peak -- the converter's ceiling.
//
// Launch shape.  One workgroup of 256 threads per row.  The recurrence is serial in the sample index; one lane per row
// would pay the whole dependent float64 chain of a 16000-sample row, so the workgroup runs it block-parallel: a span of
// 16384 samples is 256 chunks of 64, every thread filters its chunk from zero state, a log-step scan over the
// workgroup turns the 256 end states into the true carries (the powers M^(2^j) of the chunk's state matrix come from
// the bank), and every thread filters its chunk again from its true start state.  A workgroup marches over the spans
// of a long row; the last carry of a span seeds the next.
//
// LDS layout.  The span as float64, chunk t at a pitch of 65 doubles: element k of chunk t is span[65 t + k].  In the
// recurrence the 32 lanes of a ds_read_b64 group read dwords 130 t + 2 k, which fall on banks (2 t + 2 k) mod 64: 32
// distinct even banks, conflict-free, where a pitch of 64 would put all of them on one.  The coalesced load and store
// (lane l on element base + l) stay inside one chunk per wave and are conflict-free as well.  130 KiB of dynamic LDS
// for the span, 8 KiB static for the scan's two buffers, 1 KiB for the peak reduction.
//
// HBM traffic per row: the row in twice (the non-finite / silence flags, then the spans), the row out, and once more in
// and out when it clips.  The bank entry (1280 bytes) is uniform per workgroup and comes through the scalar cache.
#include "../../include/cough_amd_channel.h"

#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

constexpr int CH = COUGH_CHANNEL_CHUNK, T = COUGH_CHANNEL_THREADS, SPAN = CH * T, PITCH = CH + 1;
constexpr int MAX_SEC = COUGH_CHANNEL_MAX_SECTIONS, ENTRY = COUGH_CHANNEL_ENTRY_WORDS, REC = ENTRY / MAX_SEC, POWERS = 8;
constexpr int MAX_LEN = COUGH_CHANNEL_MAX_LENGTH;
constexpr size_t LDS_BYTES = size_t(T) * PITCH * sizeof(double);
constexpr size_t ENTRY_BYTES = size_t(ENTRY) * sizeof(double);
constexpr int DT = 64;                                                             // threads of the draw kernel
static_assert(CH == 64 && T == 256 && (1 << POWERS) == T && REC == 8 + 4 * POWERS, "the blob's layout and the scan's depth");

// ------------------------------------------------------------------------------------------ the rows
// d_out may be d_src (a row in place), so neither pointer is __restrict__.
__global__ __launch_bounds__(T) void channel_kernel(const float* src, const long long* __restrict__ row_offsets,
                                                    const int* __restrict__ lengths, const cough_channel_plan* __restrict__ plans,
                                                    const double* __restrict__ bank, int n_bank, float* out, int width) {
    extern __shared__ double span[];
    __shared__ double sc[2][2][T];             // the scan, double-buffered: [buffer][component][t]
    __shared__ double carry[MAX_SEC][2];       // the previous span's last carry per section: thread 0 alone touches it
    __shared__ float red[T];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = min(max(lengths[b], 0), MAX_LEN), m = min(n, width);
    const cough_channel_plan plan = plans[b];
    const int filter = (plan.filter >= 0 && plan.filter < n_bank) ? plan.filter : -1;
    const bool clip = plan.clip_ratio >= 0.0f && plan.clip_ratio < 1.0f;        // false for a NaN
    const float* x = src + row_offsets[b];
    float* o = out + (long long)b * width;

    if (filter < 0 && !clip) {                 // a copy, bit for bit
        for (int i = tid; i < width; i += T) o[i] = i < m ? x[i] : 0.0f;
        return;
    }

    int bad = 0, live = 0;
    for (int i = tid; i < m; i += T) {
        const float v = x[i];
        bad |= !(fabsf(v) <= 3.4028234663852886e38f);                           // NaN or Inf
        live |= v != 0.0f;
    }
    // __syncthreads_or reduces ONE predicate: the two flags take a reduction each
    const bool any_bad = __syncthreads_or(bad) != 0;
    const bool any_live = __syncthreads_or(live) != 0;
    if (any_bad || !any_live) {                // a non-finite input: NaN; silence: +0.0
        const float fill = any_bad ? __int_as_float(0x7FC00000) : 0.0f;
        for (int i = tid; i < width; i += T) o[i] = i < m ? fill : 0.0f;
        return;
    }

    float peak = 0.0f;
    if (filter < 0) {                          // the ceiling alone
        for (int i = tid; i < m; i += T) {
            const float v = x[i];
            o[i] = v;
            peak = fmaxf(peak, fabsf(v));
        }
    } else {
        const double* __restrict__ entry = bank + size_t(filter) * ENTRY;
        const int n_sec = min(max(int(entry[5]), 1), MAX_SEC);
        if (tid == 0)
            for (int s = 0; s < MAX_SEC; ++s) carry[s][0] = carry[s][1] = 0.0;
        double* mine = span + tid * PITCH;
        for (int s0 = 0; s0 < m; s0 += SPAN) {
            const int len = min(SPAN, m - s0);
            // ---- the span, read whole before any of it is written; zeros behind the row's end
            for (int i = tid; i < SPAN; i += T) span[(i >> 6) * PITCH + (i & (CH - 1))] = i < len ? double(x[s0 + i]) : 0.0;
            __syncthreads();
            const bool work = tid * CH < len;  // a chunk behind the row's end has nothing to filter: its end state is 0
            for (int sec = 0; sec < n_sec; ++sec) {
                const double* __restrict__ r = entry + sec * REC;
                const double b0 = r[0], b1 = r[1], b2 = r[2], a1 = r[3], a2 = r[4];
                // ---- 1. the chunk from zero state: its end state
                double z1 = 0.0, z2 = 0.0;
                if (work) {
#pragma unroll 8
                    for (int k = 0; k < CH; ++k) {
                        const double xv = mine[k];
                        const double y = b0 * xv + z1;
                        z1 = b1 * xv - a1 * y + z2;
                        z2 = b2 * xv - a2 * y;
                    }
                }
                // ---- 2. the previous span's carry enters chunk 0
                double in1 = 0.0, in2 = 0.0;
                if (tid == 0) {
                    in1 = carry[sec][0];
                    in2 = carry[sec][1];
                    const double e1 = (r[8] * in1 + r[9] * in2) + z1, e2 = (r[10] * in1 + r[11] * in2) + z2;
                    z1 = e1;
                    z2 = e2;
                }
                // ---- 3. the carries: an inclusive log-step scan of s[t] = M s[t-1] + e[t]
                sc[0][0][tid] = z1;
                sc[0][1][tid] = z2;
                __syncthreads();
                int cur = 0;
#pragma unroll
                for (int j = 0; j < POWERS; ++j) {
                    const int d = 1 << j;
                    double v1 = sc[cur][0][tid], v2 = sc[cur][1][tid];
                    if (tid >= d) {
                        const double p1 = sc[cur][0][tid - d], p2 = sc[cur][1][tid - d];
                        const double* __restrict__ mj = r + 8 + 4 * j;
                        const double w1 = (mj[0] * p1 + mj[1] * p2) + v1, w2 = (mj[2] * p1 + mj[3] * p2) + v2;
                        v1 = w1;
                        v2 = w2;
                    }
                    cur ^= 1;
                    sc[cur][0][tid] = v1;
                    sc[cur][1][tid] = v2;
                    __syncthreads();
                }
                // ---- 4. the chunk again, from its true start state
                if (tid == 0) {
                    z1 = in1;
                    z2 = in2;
                    carry[sec][0] = sc[cur][0][T - 1];                          // 5. the next span's carry
                    carry[sec][1] = sc[cur][1][T - 1];
                } else {
                    z1 = sc[cur][0][tid - 1];
                    z2 = sc[cur][1][tid - 1];
                }
                __syncthreads();               // sc is free for the next section
                if (work) {
#pragma unroll 8
                    for (int k = 0; k < CH; ++k) {
                        const double xv = mine[k];
                        const double y = b0 * xv + z1;
                        z1 = b1 * xv - a1 * y + z2;
                        z2 = b2 * xv - a2 * y;
                        mine[k] = y;
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < len; i += T) {
                const float y = float(span[(i >> 6) * PITCH + (i & (CH - 1))]);
                o[s0 + i] = y;
                peak = fmaxf(peak, fabsf(y));
            }
            __syncthreads();                   // the span is free for the next load
        }
    }
    for (int i = m + tid; i < width; i += T) o[i] = 0.0f;
    if (!clip) return;

    // ---- the ceiling: the row's peak (a maximum: exact in any order), then every thread rewrites what it wrote itself
    red[tid] = peak;
    __syncthreads();
    for (int h = T / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
        __syncthreads();
    }
    const float c = plan.clip_ratio * red[0];
    for (int i = tid; i < m; i += T) {
        const float y = o[i];
        o[i] = y > c ? c : (y < -c ? -c : y);
    }
}

// ------------------------------------------------------------------------------------------ the channel draws of one row
// The contract of cough_amd_channel.h, operator by operator; tests/channel_ref.py restates it in numpy.
__global__ __launch_bounds__(DT) void draw_channel_kernel(unsigned long long seed, int n_rows, double p, int n_bank, double p_clip,
                                                          double lo, double hi, cough_channel_plan* __restrict__ plans) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= n_rows) return;
    const uint2 key = make_uint2(unsigned(seed), unsigned(seed >> 32));
    auto unit = [](unsigned x) { return (double(x) + 0.5) * 0x1p-32; };
    cough_channel_plan plan;
    plan.filter = -1;
    plan.clip_ratio = 1.0f;
    const uint4 d = philox4x32_10(make_uint4(0u, unsigned(row), 0u, 5u), key);
    if (unit(d.x) <= p) {
        if (n_bank >= 1) plan.filter = min(int(double(n_bank) * unit(d.y)), n_bank - 1);
        if (unit(d.z) <= p_clip) {
            const double span_ = hi - lo;
            const double scaled = span_ * unit(d.w);
            plan.clip_ratio = float(lo + scaled);
        }
    }
    plans[row] = plan;
}

// 130 KiB of dynamic LDS is a per-device attribute of the kernel: set once per thread and device
int allow_lds() {
    thread_local int allowed_on = -1;
    int dev = 0;
    COUGH_HIP_CHECK(hipGetDevice(&dev));
    if (dev == allowed_on) return COUGH_OK;
    COUGH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&channel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(LDS_BYTES)));
    allowed_on = dev;
    return COUGH_OK;
}

// P <- X * Y, one IEEE operation per operator (the header's order)
void mat2(const double* x, const double* y, double* p) {
#pragma clang fp contract(off)
    const double p00 = x[0] * y[0] + x[1] * y[2], p01 = x[0] * y[1] + x[1] * y[3];
    const double p10 = x[2] * y[0] + x[3] * y[2], p11 = x[2] * y[1] + x[3] * y[3];
    p[0] = p00;
    p[1] = p01;
    p[2] = p10;
    p[3] = p11;
}

}  // namespace
}  // namespace cough

extern "C" int cough_channel_abi_version(void) { return COUGH_CHANNEL_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_channel_last_error)

extern "C" size_t cough_channel_bank_bytes(int n_bank) {
    if (n_bank < 0 || size_t(n_bank) > SIZE_MAX / cough::ENTRY_BYTES) return 0;
    return cough::ENTRY_BYTES * size_t(n_bank > 0 ? n_bank : 1);
}

extern "C" int cough_channel_prepare(const double* h_sos, const int* h_n_sections, int n_bank, void* d_bank, size_t bank_bytes,
                                     void* stream) {
    using namespace cough;
    const char* fn = "cough_channel_prepare";
    COUGH_REQUIRE(n_bank >= 0, COUGH_EINVAL, "%s: n_bank must not be negative, got %d", fn, n_bank);
    COUGH_REQUIRE(d_bank, COUGH_EINVAL, "%s: NULL bank", fn);
    COUGH_REQUIRE(aligned(d_bank, 256), COUGH_EINVAL, "%s: the bank must be 256-byte aligned", fn);
    const size_t need = cough_channel_bank_bytes(n_bank);
    COUGH_REQUIRE(need != 0 && bank_bytes >= need, COUGH_EWORKSPACE, "%s: the bank holds %zu bytes, %zu are needed", fn, bank_bytes,
                  need);
    if (n_bank == 0) return COUGH_OK;
    COUGH_REQUIRE(h_sos && h_n_sections, COUGH_EINVAL, "%s: NULL argument", fn);
    std::vector<double> blob(size_t(n_bank) * ENTRY, 0.0);
    const double* row = h_sos;
    for (int r = 0; r < n_bank; ++r) {
        const int ns = h_n_sections[r];
        COUGH_REQUIRE(ns >= 1 && ns <= MAX_SEC, COUGH_EINVAL, "%s: entry %d has %d sections (1..%d)", fn, r, ns, MAX_SEC);
        double* entry = blob.data() + size_t(r) * ENTRY;
        for (int s = 0; s < ns; ++s, row += 6) {
            for (int k = 0; k < 6; ++k)
                COUGH_REQUIRE(std::isfinite(row[k]), COUGH_EINVAL, "%s: entry %d, section %d holds a NaN or an Inf", fn, r, s);
            COUGH_REQUIRE(row[3] != 0.0, COUGH_EINVAL, "%s: entry %d, section %d has a0 = 0", fn, r, s);
            double* rec = entry + s * REC;
            const double a0 = row[3];
            rec[0] = row[0] / a0;
            rec[1] = row[1] / a0;
            rec[2] = row[2] / a0;
            rec[3] = row[4] / a0;
            rec[4] = row[5] / a0;
            for (int k = 0; k < 5; ++k)
                COUGH_REQUIRE(std::isfinite(rec[k]), COUGH_EINVAL, "%s: entry %d, section %d overflows when divided by a0", fn, r, s);
            const double a1 = rec[3], a2 = rec[4];
            COUGH_REQUIRE(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2, COUGH_EINVAL,
                          "%s: entry %d, section %d is not stable (a1 = %g, a2 = %g)", fn, r, s, a1, a2);
            double p[4] = {-a1, 1.0, -a2, 0.0};                                 // A
            for (int q = 0; q < 6; ++q) mat2(p, p, p);                          // A^64 = M
            for (int j = 0; j < POWERS; ++j) {
                for (int k = 0; k < 4; ++k) rec[8 + 4 * j + k] = p[k];
                mat2(p, p, p);
            }
        }
        entry[5] = double(ns);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    COUGH_HIP_CHECK(hipMemcpyAsync(d_bank, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice, st));
    COUGH_HIP_CHECK(hipStreamSynchronize(st));       // the blob is a local: it must outlive the copy
    return COUGH_OK;
}

extern "C" int cough_channel_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                  const cough_channel_plan* d_plans, const void* d_bank, int n_bank, float* d_out, int width,
                                  void* stream) {
    using namespace cough;
    const char* fn = "cough_channel_rows";
    COUGH_REQUIRE(n_rows >= 0 && width >= 1 && n_bank >= 0, COUGH_EINVAL, "%s: bad sizes (%d rows of %d columns, %d filters)", fn,
                  n_rows, width, n_bank);
    COUGH_REQUIRE(width <= MAX_LEN, COUGH_EUNSUPPORTED, "%s: width = %d is more than 2^30", fn, width);
    COUGH_REQUIRE(n_rows <= (1 << 24), COUGH_EUNSUPPORTED, "%s: %d rows are more than 2^24 blocks; split the batch", fn, n_rows);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_plans && d_out && (d_bank || n_bank == 0), COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4) && aligned(d_plans, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8) && aligned(d_bank, 256), COUGH_EINVAL,
                  "%s: d_row_offsets must be 8-byte and the bank 256-byte aligned", fn);
    if (const int e = allow_lds()) return e;
    hipLaunchKernelGGL(channel_kernel, dim3(unsigned(n_rows)), dim3(T), LDS_BYTES, static_cast<hipStream_t>(stream), d_src,
                       d_row_offsets, d_lengths, d_plans, static_cast<const double*>(d_bank), n_bank, d_out, width);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_draw_channel(unsigned long long seed, int n_rows, double p_augment, int n_bank, double p_clip, double clip_lo,
                                  double clip_hi, cough_channel_plan* d_plans_out, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_channel";
    COUGH_REQUIRE(n_rows >= 0 && n_bank >= 0, COUGH_EINVAL, "%s: bad sizes (%d rows, %d filters)", fn, n_rows, n_bank);
    COUGH_REQUIRE(p_augment >= 0.0 && p_augment <= 1.0, COUGH_EINVAL, "%s: p_augment = %g (0..1)", fn, p_augment);
    COUGH_REQUIRE(p_clip >= 0.0 && p_clip <= 1.0, COUGH_EINVAL, "%s: p_clip = %g (0..1)", fn, p_clip);
    COUGH_REQUIRE(std::isfinite(clip_lo) && std::isfinite(clip_hi) && clip_lo <= clip_hi, COUGH_EINVAL,
                  "%s: the clip range (%g, %g) must be finite and ordered", fn, clip_lo, clip_hi);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_plans_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_plans_out, 4), COUGH_EINVAL, "%s: the plans must be 4-byte aligned", fn);
    hipLaunchKernelGGL(draw_channel_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream),
                       seed, n_rows, p_augment, n_bank, p_clip, clip_lo, clip_hi, d_plans_out);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
