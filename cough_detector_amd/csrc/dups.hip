// libcough_amd_dups.so: binary fingerprints of feature images and the all-pairs matcher over them
// (include/cough_amd_dups.h, which states the arithmetic).  Three kernels and a small scan.
//
// Fingerprint.  One workgroup per clip, thread t owns frame t: it sums W columns of each of the 33 rows at t and at
// t + D straight from global memory (adjacent threads read adjacent columns; a clip's 33 rows stay in L1 / L2 between
// the W + D passes over them), keeps the previous row's two sums, and forms one bit per row pair.  Nothing is staged:
// the kernel is bound by the one pass over the rows that reaches HBM.
//
// Matcher.  One workgroup per tile of 64 x 64 clip pairs (tiles below the diagonal return at once).  Both sets of words
// are staged in LDS frame-major, [t][64 clips], and each thread owns a 4 x 4 block of pairs -- clips 4 ty .. 4 ty + 3 of
// the a tile, 4 tx .. 4 tx + 3 of the b tile -- so one step is two ds_read_b128 (a lane group of that instruction holds
// every tx once and two ty: the b side reads the 16 slots of one 256-byte bank row, the a side two of them) for 16 XOR
// + popcount-accumulate, and every address is the loop's base plus a constant.  (An odd row pitch, clip-major, was
// measured first: 8 ds_read_b32 and their address arithmetic per step, 50 VALU instructions per step instead of 40;
// profiles/dups_bench.txt.)  Staging writes a clip's frames 64 words apart, all on one bank: those conflicts are more
// than half of the LDS array's cycles, and the array is still busy well under half of the time -- VALU issue bounds
// the kernel, not LDS.  The live count never
// enters that loop: a met frame is dead iff both words are zero, so staging also leaves a bitmap of each row's zero
// words (a ballot per 64 frames), and the dead frames of a pair at a lag are popcounts of za & (zb >> lag), 3 words at
// Tw = 86.  Per-tile match counts of every row go to a place of their own in the workspace; a scan turns them into the
// offsets the list pass writes to.  The list pass repeats the arithmetic of a tile only where the counts say the tile
// holds a match, and orders a row's matches by ballot prefixes: no atomics but the histogram's integer additions.
#include "../../include/cough_amd_dups.h"

#include "common.h"

namespace cough {

namespace {

constexpr int FP_THREADS = 256;              // >= COUGH_DUPS_MAX_FRAMES: thread t owns frame t
constexpr int TILE = 64;                     // clips of a tile's side
constexpr int RB = 4;                        // a thread's pairs: RB x RB
constexpr int SIDE = TILE / RB;              // 16 x 16 threads
constexpr int MATCH_THREADS = SIDE * SIDE;
constexpr int MASK_WORDS = COUGH_DUPS_MAX_FRAMES / 32;   // a row's zero-word bitmap
constexpr size_t DEFAULT_DYNAMIC_LDS = 64 * 1024;        // what a kernel gets without hipFuncSetAttribute
static_assert(FP_THREADS >= COUGH_DUPS_MAX_FRAMES && MATCH_THREADS == 256 && TILE == 64, "thread maps below");

struct RowTable {
    int r[COUGH_DUPS_ROWS];
};

__global__ __launch_bounds__(FP_THREADS) void fingerprint_kernel(const float* __restrict__ images, int F, int T, RowTable rows,
                                                                 int W, int D, int Tw, unsigned* __restrict__ words,
                                                                 int* __restrict__ live) {
    __shared__ int s_live[FP_THREADS / 64];
    const int clip = blockIdx.x, t = threadIdx.x;
    const float* image = images + size_t(clip) * size_t(F) * size_t(T);
    unsigned word = 0;
    if (t < Tw) {                                                // the last column read is t + D + W - 1 <= T - 1
        float prev_a = 0.f, prev_b = 0.f;
#pragma unroll
        for (int k = 0; k < COUGH_DUPS_ROWS; ++k) {
            const float* row = image + size_t(rows.r[k]) * size_t(T) + t;
            float sum_a = row[0], sum_b = row[D];
            for (int j = 1; j < W; ++j) {
                sum_a = sum_a + row[j];
                sum_b = sum_b + row[D + j];
            }
            if (k > 0) {
                const float d_a = prev_a - sum_a, d_b = prev_b - sum_b;
                if ((d_b - d_a) > 0.0f) word |= 1u << (k - 1);
            }
            prev_a = sum_a;
            prev_b = sum_b;
        }
        words[size_t(clip) * size_t(Tw) + t] = word;
    }
    const int alive = __popcll(__ballot(word != 0));
    if ((t & 63) == 0) s_live[t >> 6] = alive;
    __syncthreads();
    if (t == 0) live[clip] = s_live[0] + s_live[1] + s_live[2] + s_live[3];
}

struct MatchParams {
    int n, Tw, L, max_err_1024, min_live, n_tiles;
};

__host__ __device__ inline int tiles_of(int n) { return (n + TILE - 1) / TILE; }
inline size_t match_shared_bytes(int Tw) {
    return sizeof(unsigned) * (size_t(2) * TILE * Tw + 2 * TILE * MASK_WORDS + COUGH_DUPS_HIST_BINS + 1);
}

// acc + popcount(x) as the one instruction it is.  Written as `acc += __popc(x)` the unrolled loop is reassociated into
// counts from zero and v_add3_u32 trees: 3 instructions per 2 steps where v_bcnt_u32_b32 adds for nothing.
__device__ __forceinline__ int popc_add(int acc, unsigned x) {
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
    return acc;
}

// the zero bitmap of row `z`, moved so that bit t of word w is the row's bit 32 w + t + lag (lag = 32 q + r, 0 <= r < 32)
__device__ __forceinline__ unsigned moved_mask(const unsigned* z, int w, int q, int r) {
    const int lo = w + q, hi = lo + 1;
    const unsigned a = lo >= 0 && lo < MASK_WORDS ? z[lo] : 0u;
    const unsigned b = hi >= 0 && hi < MASK_WORDS ? z[hi] : 0u;
    return r ? (a >> r) | (b << (32 - r)) : a;
}

// The workspace: int32 [n_tiles + 1][n_pad], n_pad = 64 n_tiles.  After the count pass entry [tb][a] is clip a's matches
// in tile tb of b; after the scan it is the matches in front of that tile, and [n_tiles][a] the total.
template <bool LIST>
__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(const unsigned* __restrict__ words, const int* __restrict__ live,
                                                              MatchParams p, int* ws, unsigned long long* hist,
                                                              const long long* __restrict__ row_offs, int* __restrict__ out_a,
                                                              int* __restrict__ out_b, int* __restrict__ out_lag,
                                                              int* __restrict__ out_err, int* __restrict__ out_bits) {
    extern __shared__ __align__(16) unsigned smem[];
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (tb < ta) return;                                         // every pair of the tile has a > b
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Tw = p.Tw;
    const size_t n_pad = size_t(p.n_tiles) * TILE;
    unsigned* sa = smem;
    unsigned* sb = sa + TILE * Tw;                               // [t][clip], 256 bytes per frame
    unsigned* za = sb + TILE * Tw;
    unsigned* zb = za + TILE * MASK_WORDS;
    int* s_hist = reinterpret_cast<int*>(zb + TILE * MASK_WORDS);

    if (LIST) {                                                  // a tile without a match is not computed again
        int here = 0;
        if (tid < TILE && ta * TILE + tid < p.n) {
            const size_t a = size_t(ta) * TILE + tid;
            here = ws[size_t(tb + 1) * n_pad + a] - ws[size_t(tb) * n_pad + a];
        }
        if (!__syncthreads_or(here)) return;
    }

    // staging: a wave per row, 64 frames per load, and the row's zero words as a ballot
    for (int r = wave; r < 2 * TILE; r += MATCH_THREADS / 64) {
        const bool second = r >= TILE;
        const int local = r & (TILE - 1);
        const int clip = (second ? tb : ta) * TILE + local;
        unsigned* dst = (second ? sb : sa) + local;
        unsigned* z = (second ? zb : za) + local * MASK_WORDS;
#pragma unroll
        for (int c = 0; c < COUGH_DUPS_MAX_FRAMES / 64; ++c) {
            const int t = c * 64 + lane;
            const bool in = t < Tw;
            unsigned w = 0;
            if (in && clip < p.n) w = words[size_t(clip) * size_t(Tw) + t];
            if (in) dst[t * TILE] = w;
            const unsigned long long zero = __ballot(in && w == 0);
            if (lane == 0) {
                z[2 * c] = unsigned(zero);
                z[2 * c + 1] = unsigned(zero >> 32);
            }
        }
    }
    if (!LIST && tid < COUGH_DUPS_HIST_BINS) s_hist[tid] = 0;
    __syncthreads();

    const int tx = tid & (SIDE - 1), ty = tid >> 4;
    bool valid[RB][RB];
    {
        int live_a[RB], live_b[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int a = ta * TILE + RB * ty + i, b = tb * TILE + RB * tx + i;
            live_a[i] = a < p.n ? live[a] : 0;
            live_b[i] = b < p.n ? live[b] : 0;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < RB; ++j)
                valid[i][j] = ta * TILE + RB * ty + i < tb * TILE + RB * tx + j && live_a[i] > 0 && live_b[j] > 0;
    }

    int best_err[RB][RB], best_bits[RB][RB], best_lag[RB][RB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < RB; ++j) best_err[i][j] = best_bits[i][j] = best_lag[i][j] = 0;

    const int L = min(p.L, Tw - 1);                              // a longer lag meets no frame
    const int mask_words = (Tw + 31) >> 5;
    const uint4* rows_a = reinterpret_cast<const uint4*>(sa + RB * ty);          // frame t: rows_a[t * SIDE]
    const unsigned* mask_a = za + RB * ty * MASK_WORDS;
    const unsigned* mask_b = zb + RB * tx * MASK_WORDS;
    for (int visit = 0; visit <= 2 * L; ++visit) {               // 0, -1, +1, -2, +2, ...
        const int lag = visit == 0 ? 0 : (visit & 1) ? -((visit + 1) >> 1) : visit >> 1;
        const int t0 = max(0, -lag), t1 = min(Tw, Tw - lag);
        const uint4* rows_b = reinterpret_cast<const uint4*>(sb + RB * tx) + lag * SIDE;
        int err[RB][RB], dead[RB][RB];
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < RB; ++j) err[i][j] = dead[i][j] = 0;
#pragma clang loop vectorize(disable) unroll_count(4)
        for (int t = t0; t < t1; ++t) {
            const uint4 a4 = rows_a[t * SIDE], b4 = rows_b[t * SIDE];
            const unsigned av[RB] = {a4.x, a4.y, a4.z, a4.w}, bv[RB] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) err[i][j] = popc_add(err[i][j], av[i] ^ bv[j]);
        }
        const int q = lag >> 5, r = lag & 31;                    // floor and remainder, also for a negative lag
        for (int w = 0; w < mask_words; ++w) {
            unsigned zav[RB], zbv[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                zav[i] = mask_a[i * MASK_WORDS + w];
                zbv[i] = moved_mask(mask_b + i * MASK_WORDS, w, q, r);
            }
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) dead[i][j] += __popc(zav[i] & zbv[j]);
        }
        const int met = t1 - t0;
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int frames = met - dead[i][j];
                const int bits = 32 * frames, e = err[i][j];
                const bool better = best_bits[i][j] == 0 || e * best_bits[i][j] < best_err[i][j] * bits;
                if (valid[i][j] && frames >= p.min_live && better) {
                    best_err[i][j] = e;
                    best_bits[i][j] = bits;
                    best_lag[i][j] = lag;
                }
            }
    }

    // a clip of the a tile is the 16 lanes of one ty in its wave; its matches in ascending b are tx first, then j
    const int shift = 16 * ((lane >> 4) & 3);
    const unsigned lower = (1u << tx) - 1u;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int a = ta * TILE + RB * ty + i;
        long long base = 0, end = 0;
        if (LIST && a < p.n) {
            base = row_offs[a] + ws[size_t(tb) * n_pad + a];
            end = row_offs[a + 1];
        }
        bool match[RB];
        int total = 0, before = 0;                               // the row's matches; those of the lanes with a smaller tx
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const bool has = best_bits[i][j] > 0;
            match[j] = has && best_err[i][j] * 1024 <= p.max_err_1024 * best_bits[i][j];
            const unsigned mine = unsigned(__ballot(match[j]) >> shift) & 0xFFFFu;
            total += __popc(mine);
            before += __popc(mine & lower);
            if (!LIST && has) atomicAdd(&s_hist[(best_err[i][j] * 64) / best_bits[i][j]], 1);
        }
        if (LIST) {
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const long long at = base + before;
                if (match[j] && at >= 0 && at < end) {
                    out_a[at] = a;
                    out_b[at] = tb * TILE + RB * tx + j;
                    out_lag[at] = best_lag[i][j];
                    out_err[at] = best_err[i][j];
                    out_bits[at] = best_bits[i][j];
                }
                before += match[j] ? 1 : 0;
            }
        } else if (tx == 0 && a < p.n) {
            ws[size_t(tb) * n_pad + a] = total;
        }
    }
    if (!LIST) {
        __syncthreads();
        if (tid < COUGH_DUPS_HIST_BINS && s_hist[tid]) atomicAdd(&hist[tid], (unsigned long long)s_hist[tid]);
    }
}

// per clip: counts of the tiles tb >= ta -> what lies in front of each tile, the total behind them and in d_counts
__global__ __launch_bounds__(256) void scan_counts_kernel(int* ws, int n, int n_tiles, int* __restrict__ counts) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const size_t n_pad = size_t(n_tiles) * TILE;
    int run = 0;
    for (int tb = a / TILE; tb < n_tiles; ++tb) {
        const int c = ws[size_t(tb) * n_pad + a];
        ws[size_t(tb) * n_pad + a] = run;
        run += c;
    }
    ws[size_t(n_tiles) * n_pad + a] = run;
    counts[a] = run;
}

int check_match(const char* fn, const void* d_words, const void* d_live, int n, int Tw, int L, int max_err_1024, int min_live,
                const void* d_workspace, size_t workspace_bytes) {
    COUGH_REQUIRE(n >= 0 && n <= COUGH_DUPS_MAX_CLIPS, COUGH_EINVAL, "%s: n = %d must lie in 0..%d (more clips are refused, not truncated)",
                  fn, n, COUGH_DUPS_MAX_CLIPS);
    COUGH_REQUIRE(Tw >= 1 && Tw <= COUGH_DUPS_MAX_FRAMES, COUGH_EINVAL, "%s: Tw = %d must lie in 1..%d", fn, Tw,
                  COUGH_DUPS_MAX_FRAMES);
    COUGH_REQUIRE(L >= 0, COUGH_EINVAL, "%s: the largest lag L must not be negative, got %d", fn, L);
    COUGH_REQUIRE(max_err_1024 >= 0 && max_err_1024 <= 1024, COUGH_EINVAL, "%s: max_err_1024 = %d must lie in 0..1024", fn,
                  max_err_1024);
    COUGH_REQUIRE(min_live >= 1, COUGH_EINVAL, "%s: min_live must be positive, got %d", fn, min_live);
    COUGH_REQUIRE(d_words && d_live && d_workspace, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_words, 4) && aligned(d_live, 4), COUGH_EINVAL, "%s: 32-bit arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_workspace, 256), COUGH_EINVAL, "%s: the workspace must be 256-byte aligned", fn);
    COUGH_REQUIRE(workspace_bytes >= cough_match_workspace_bytes(n, Tw), COUGH_EWORKSPACE,
                  "%s: the workspace holds %zu bytes, %zu are needed", fn, workspace_bytes, cough_match_workspace_bytes(n, Tw));
    return COUGH_OK;
}

template <bool LIST>
int allow_lds(size_t bytes) {
    if (bytes > DEFAULT_DYNAMIC_LDS)
        COUGH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&match_kernel<LIST>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
    return COUGH_OK;
}

}  // namespace
}  // namespace cough

extern "C" int cough_dups_abi_version(void) { return COUGH_DUPS_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_dups_last_error)

extern "C" int cough_fingerprint_images(const float* d_images, int n, int F, int T, const int* rows, int window, int delta,
                                        unsigned int* d_words, int* d_live, void* stream) {
    using namespace cough;
    const char* fn = "cough_fingerprint_images";
    COUGH_REQUIRE(d_images && rows && d_words && d_live, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n >= 0, COUGH_EINVAL, "%s: n must not be negative, got %d", fn, n);
    COUGH_REQUIRE(F >= 1 && T >= 1, COUGH_EINVAL, "%s: the images must have rows and columns, got F = %d, T = %d", fn, F, T);
    COUGH_REQUIRE(window >= 1, COUGH_EINVAL, "%s: window must be positive, got %d", fn, window);
    COUGH_REQUIRE(delta >= 1, COUGH_EINVAL, "%s: delta must be positive, got %d", fn, delta);
    const long long Tw = (long long)T - window + 1 - delta;
    COUGH_REQUIRE(Tw >= 1 && Tw <= COUGH_DUPS_MAX_FRAMES, COUGH_EINVAL,
                  "%s: Tw = T - window + 1 - delta = %lld must lie in 1..%d (T = %d, window = %d, delta = %d)", fn, Tw,
                  COUGH_DUPS_MAX_FRAMES, T, window, delta);
    RowTable table;
    for (int k = 0; k < COUGH_DUPS_ROWS; ++k) {
        COUGH_REQUIRE(rows[k] >= 0 && rows[k] < F, COUGH_EINVAL, "%s: rows[%d] = %d lies outside the image's rows 0..%d", fn, k,
                      rows[k], F - 1);
        table.r[k] = rows[k];
    }
    COUGH_REQUIRE(aligned(d_images, 4) && aligned(d_words, 4) && aligned(d_live, 4), COUGH_EINVAL,
                  "%s: 32-bit arrays must be 4-byte aligned", fn);
    if (n == 0) return COUGH_OK;
    hipLaunchKernelGGL(fingerprint_kernel, dim3(unsigned(n)), dim3(FP_THREADS), 0, static_cast<hipStream_t>(stream), d_images,
                       F, T, table, window, delta, int(Tw), d_words, d_live);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" size_t cough_match_workspace_bytes(int n, int Tw) {
    if (n < 1 || n > COUGH_DUPS_MAX_CLIPS || Tw < 1 || Tw > COUGH_DUPS_MAX_FRAMES) return 0;
    const size_t tiles = size_t(cough::tiles_of(n));
    return sizeof(int) * tiles * cough::TILE * (tiles + 1);
}

extern "C" int cough_count_matches(const unsigned int* d_words, const int* d_live, int n, int Tw, int L, int max_err_1024,
                                   int min_live, int* d_counts, long long* d_hist, void* d_workspace, size_t workspace_bytes,
                                   void* stream) {
    using namespace cough;
    const char* fn = "cough_count_matches";
    if (int rc = check_match(fn, d_words, d_live, n, Tw, L, max_err_1024, min_live, d_workspace, workspace_bytes)) return rc;
    COUGH_REQUIRE(d_counts && d_hist, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_counts, 4), COUGH_EINVAL, "%s: 32-bit arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_hist, 8), COUGH_EINVAL, "%s: the int64 histogram must be 8-byte aligned", fn);
    if (n == 0) return COUGH_OK;
    const size_t lds = match_shared_bytes(Tw);
    if (int rc = allow_lds<false>(lds)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MatchParams p{n, Tw, L, max_err_1024, min_live, tiles_of(n)};
    COUGH_HIP_CHECK(hipMemsetAsync(d_hist, 0, sizeof(long long) * COUGH_DUPS_HIST_BINS, s));
    hipLaunchKernelGGL(match_kernel<false>, dim3(unsigned(p.n_tiles), unsigned(p.n_tiles)), dim3(MATCH_THREADS), lds, s, d_words,
                       d_live, p, static_cast<int*>(d_workspace), reinterpret_cast<unsigned long long*>(d_hist),
                       static_cast<const long long*>(nullptr), static_cast<int*>(nullptr), static_cast<int*>(nullptr),
                       static_cast<int*>(nullptr), static_cast<int*>(nullptr), static_cast<int*>(nullptr));
    COUGH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scan_counts_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, static_cast<int*>(d_workspace), n,
                       p.n_tiles, d_counts);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_list_matches(const unsigned int* d_words, const int* d_live, int n, int Tw, int L, int max_err_1024,
                                  int min_live, const void* d_workspace, size_t workspace_bytes,
                                  const long long* d_row_offsets, int* d_a, int* d_b, int* d_lag, int* d_err, int* d_bits,
                                  void* stream) {
    using namespace cough;
    const char* fn = "cough_list_matches";
    if (int rc = check_match(fn, d_words, d_live, n, Tw, L, max_err_1024, min_live, d_workspace, workspace_bytes)) return rc;
    COUGH_REQUIRE(d_row_offsets && d_a && d_b && d_lag && d_err && d_bits, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_a, 4) && aligned(d_b, 4) && aligned(d_lag, 4) && aligned(d_err, 4) && aligned(d_bits, 4),
                  COUGH_EINVAL, "%s: 32-bit arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8), COUGH_EINVAL, "%s: the int64 row offsets must be 8-byte aligned", fn);
    if (n == 0) return COUGH_OK;
    const size_t lds = match_shared_bytes(Tw);
    if (int rc = allow_lds<true>(lds)) return rc;
    const MatchParams p{n, Tw, L, max_err_1024, min_live, tiles_of(n)};
    hipLaunchKernelGGL(match_kernel<true>, dim3(unsigned(p.n_tiles), unsigned(p.n_tiles)), dim3(MATCH_THREADS), lds,
                       static_cast<hipStream_t>(stream), d_words, d_live, p,
                       const_cast<int*>(static_cast<const int*>(d_workspace)), static_cast<unsigned long long*>(nullptr),
                       d_row_offsets, d_a, d_b, d_lag, d_err, d_bits);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
