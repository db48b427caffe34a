// Exact error quantiles of a disparity map against ground truth, on the device (include/mccnn.h:
// mccnn_evaluate_quantiles, mccnn_evaluate_quantiles_pooled); the text in the header is the definition.
//
// Regions, validity and error are those of mccnn_evaluate (csrc/evaluate.hip).  A scored pixel's key is the bit pattern of
// err = fabsf(disp - gt); for non-negative floats the key order is the value order, so the nearest-rank quantile is the
// key of rank r among the region's scored pixels.  It is found by a most-significant-digit radix selection with four
// 8-bit digits; every pass recomputes err from disp, gt and mask (9 bytes per pixel), no error map is stored:
//   memset               the histograms in scratch
//   quantile_hist<0>     the top digit of every scored pixel, per region: 2 x 256 bins shared by all quantiles; the same
//                        read feeds the list's pool (key >> 16, 64-bit counts) when the caller gave one
//   quantile_select(0)   one workgroup: n_scored = the histogram's total, the ranks from n_scored and q_ppm in 64-bit
//                        integers, then per target (region x quantile, up to 16) the bin that holds its rank and the rank
//                        left inside that bin
//   quantile_hist<p>     p = 1, 2, 3: the next digit among the pixels whose upper digits equal a target's prefix, one
//                        histogram of 256 bins per target (a pixel that matches several targets counts for each)
//   quantile_select(p)   the next digit of every target; after the last digit the prefix IS the key: result is written
// Nothing travels to the host between the launches.  Only integer atomics touch memory (LDS and global); integer sums
// commute, so a call and a replayed graph give the same bits whatever order the workgroups arrive in.
//
// A workgroup keeps its histograms in LDS (2 KB in the first pass, 16 KB in the later ones) and flushes the non-zero bins
// with one global atomic each; the grid is capped and strides over the map.  The pool's 2 x 65536 bins do not fit LDS:
// a workgroup combines them in a direct-mapped LDS table of 2 x 2048 (bin, count) slots indexed by the bin's low eleven
// bits - sixteen octaves of error apart before two bins meet in a slot - and a pixel whose slot belongs to another bin
// adds to the pool directly.  Errors cluster, so nearly every add stays in LDS.
#include <math.h>

#include "common.h"

namespace mccnn {
namespace {

constexpr int kQThreads = 256;
constexpr int kQWaves = kQThreads / kWave;
constexpr int kQTerms = 4;                                   // pixels per thread and grid stride
constexpr int kQMaxGrid = 2048;
constexpr int kQ = MCCNN_EVAL_MAX_QUANTILES;
constexpr int kTargets = 2 * kQ;                             // region-major: all 0..7, nonocc 8..15
constexpr int kBins = 256;
constexpr int kPasses = 4;
constexpr int kPoolBins = 65536;
constexpr int kPoolSlots = 2048;
constexpr uint32_t kEmptySlot = 0xffffffffu;                 // no bin: a bin is below 65536
constexpr uint32_t kNaNBits = 0x7fc00000u;
constexpr uint64_t kQMaxPixels = 4294967295ull;              // the bin counts are uint32

static_assert(sizeof(mccnn_quantile_region_t) == 104 && sizeof(mccnn_eval_quantiles_t) == 208, "mccnn_eval_quantiles_t layout");
static_assert(MCCNN_EVAL_POOL_BYTES == 2 * kPoolBins * 8, "pool layout");

struct Quantiles {
    uint32_t ppm[kQ];
};

// What the select kernels hand from one pass to the next, at the head of scratch; the histograms follow.
struct SelectState {
    uint64_t n[2];               // scored pixels per region
    uint64_t rank[kTargets];     // the target's rank in its region
    uint64_t left[kTargets];     // ... and inside the bins chosen so far
    uint32_t prefix[kTargets];   // the digits chosen so far, right-aligned
};

constexpr size_t kStateBytes = (sizeof(SelectState) + 15) & ~(size_t)15;
constexpr size_t kHist0 = 2 * kBins;                         // uint32 words of pass 0
constexpr size_t kHistP = kTargets * kBins;                  // ... of each later pass
constexpr size_t kHistBytes = (kHist0 + (kPasses - 1) * kHistP) * sizeof(uint32_t);
constexpr size_t kScratchBytes = kStateBytes + kHistBytes;

inline uint32_t *hist_of(void *scratch, int pass)
{
    uint32_t *h = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + kStateBytes);
    return pass == 0 ? h : h + kHist0 + (size_t)(pass - 1) * kHistP;
}

// A pixel of the map: whether each region scores it, and its key.
struct Pixel {
    bool scored[2];
    uint32_t key;
};

__device__ __forceinline__ Pixel load_pixel(const float *__restrict__ disp, const float *__restrict__ gt,
                                            const uint8_t *__restrict__ mask, size_t i, size_t n)
{
    const bool inside = i < n;
    const float g = inside ? gt[i] : INFINITY;
    const float d = inside ? disp[i] : 0.f;
    const uint32_t m = (inside && mask) ? mask[i] : 255u;
    const bool in_all = inside && isfinite(g);
    const bool valid = isfinite(d) && !(d < 0.f);
    Pixel p;
    p.scored[0] = in_all && valid;
    p.scored[1] = p.scored[0] && m == 255u;
    p.key = __float_as_uint(fabsf(d - g));
    return p;
}

// PASS 0: hist[2][256], the top digit per region, and (POOL) the pool's bins.  PASS 1..3: hist[16][256], the digit at
// bit 24 - 8 * PASS of the pixels whose bits above it equal the target's prefix.  HIST == false: the pool alone.
template <int PASS, bool HIST, bool POOL>
__global__ __launch_bounds__(kQThreads) void quantile_hist_kernel(const float *__restrict__ disp, const float *__restrict__ gt,
                                                                  const uint8_t *__restrict__ mask, size_t n, int n_q,
                                                                  const SelectState *__restrict__ state,
                                                                  uint32_t *__restrict__ hist,
                                                                  unsigned long long *__restrict__ pool)
{
    constexpr int kLocal = !HIST ? 1 : PASS == 0 ? 2 * kBins : kTargets * kBins;
    constexpr int kSlots = POOL ? kPoolSlots : 1;
    constexpr int kShift = 24 - 8 * PASS;
    __shared__ uint32_t h[kLocal];
    __shared__ uint32_t slot_bin[2][kSlots], slot_count[2][kSlots];
    __shared__ uint32_t prefix[kTargets];
    const int tid = threadIdx.x;

    if (HIST) {
        for (int i = tid; i < kLocal; i += kQThreads) h[i] = 0;
        if (PASS > 0 && tid < kTargets) prefix[tid] = state->prefix[tid];
    }
    if (POOL) {
        for (int i = tid; i < 2 * kSlots; i += kQThreads) {
            (&slot_bin[0][0])[i] = kEmptySlot;
            (&slot_count[0][0])[i] = 0;
        }
    }
    __syncthreads();

    const size_t stride = (size_t)gridDim.x * (kQThreads * kQTerms);
    for (size_t base = (size_t)blockIdx.x * (kQThreads * kQTerms); base < n; base += stride) {
        Pixel px[kQTerms];
#pragma unroll
        for (int e = 0; e < kQTerms; ++e) px[e] = load_pixel(disp, gt, mask, base + (size_t)e * kQThreads + tid, n);
#pragma unroll
        for (int e = 0; e < kQTerms; ++e) {
            const uint32_t key = px[e].key;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (!px[e].scored[r]) continue;
                if (HIST && PASS == 0) atomicAdd(&h[r * kBins + (key >> 24)], 1u);
                if (HIST && PASS > 0) {
                    const uint32_t upper = key >> (kShift + 8), digit = (key >> kShift) & (kBins - 1);
                    for (int k = 0; k < n_q; ++k) {
                        if (prefix[r * kQ + k] == upper) atomicAdd(&h[(r * kQ + k) * kBins + digit], 1u);
                    }
                }
                if (POOL) {
                    const uint32_t bin = key >> 16, slot = bin & (kPoolSlots - 1);
                    const uint32_t owner = atomicCAS(&slot_bin[r][slot], kEmptySlot, bin);
                    if (owner == kEmptySlot || owner == bin)
                        atomicAdd(&slot_count[r][slot], 1u);
                    else
                        atomicAdd(&pool[(size_t)r * kPoolBins + bin], 1ull);
                }
            }
        }
    }
    __syncthreads();

    if (HIST) {
        for (int i = tid; i < kLocal; i += kQThreads) {
            const uint32_t v = h[i];
            if (v) atomicAdd(&hist[i], v);
        }
    }
    if (POOL) {
        for (int i = tid; i < 2 * kSlots; i += kQThreads) {
            const uint32_t v = (&slot_count[0][0])[i];
            if (v) atomicAdd(&pool[(size_t)(i / kSlots) * kPoolBins + (&slot_bin[0][0])[i]], (unsigned long long)v);
        }
    }
}

// r = max(ceil(q_ppm * n / 10^6) - 1, 0); n < 2^32 and q_ppm <= 10^6, so the product is below 2^52.
__device__ __forceinline__ uint64_t rank_of(uint32_t q_ppm, uint64_t n)
{
    return n ? ((uint64_t)q_ppm * n + 999999ull) / 1000000ull - 1ull : 0ull;
}

__device__ __forceinline__ void write_entry(mccnn_quantile_region_t *reg, int k, uint64_t rank, uint32_t bits)
{
    reg->rank[k] = rank;
    reinterpret_cast<uint32_t *>(reg->value)[k] = bits;      // the key itself: no float move may touch a NaN's bits
}

// Inclusive scan of one value per lane over the wave.
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t up = __shfl_up(v, d, kWave);
        if (lane >= d) v += up;
    }
    return v;
}

// One workgroup; a wave per target, four bins per lane.  pass 0 reads the region's histogram, fixes n_scored and the
// ranks; every pass picks the bin that holds the rank left; the last one writes result.
__global__ __launch_bounds__(kQThreads) void quantile_select_kernel(const uint32_t *__restrict__ hist, int pass, Quantiles q,
                                                                    int n_q, SelectState *__restrict__ state,
                                                                    mccnn_eval_quantiles_t *__restrict__ result)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool last = pass == kPasses - 1;
    for (int t = wave; t < kTargets; t += kQWaves) {             // wave-uniform
        const int r = t / kQ, k = t % kQ;
        mccnn_quantile_region_t *reg = r == 0 ? &result->all : &result->nonocc;
        if (k >= n_q) {
            if (last && lane == 0) write_entry(reg, k, 0, 0u);
            continue;
        }
        const uint32_t *h = hist + (size_t)(pass == 0 ? r : t) * kBins + lane * 4;
        const uint32_t c[4] = {h[0], h[1], h[2], h[3]};
        const uint64_t local = (uint64_t)c[0] + c[1] + c[2] + c[3];
        const uint64_t incl = wave_scan(local, lane);
        uint64_t n, left;
        uint32_t prefix = 0;
        if (pass == 0) {
            n = __shfl(incl, kWave - 1, kWave);
            left = rank_of(q.ppm[k], n);
            if (lane == 0) {
                if (k == 0) state->n[r] = n;
                state->rank[t] = left;
            }
        } else {
            n = state->n[r];
            left = state->left[t];
            prefix = state->prefix[t];
        }
        if (last && lane == 0 && k == 0) reg->n_scored = n;
        if (n == 0) {
            if (last && lane == 0) write_entry(reg, k, 0, kNaNBits);
            continue;
        }
        uint64_t below = incl - local;
        if (left >= below && left < incl) {                      // one lane: left < n, the total of the bins
            int b = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (b == j && left >= below + c[j]) {
                    below += c[j];
                    b = j + 1;
                }
            }
            const uint32_t chosen = (prefix << 8) | (uint32_t)(lane * 4 + b);
            if (!last) {
                state->prefix[t] = chosen;
                state->left[t] = left - below;
            } else {
                write_entry(reg, k, state->rank[t], chosen);
            }
        }
    }
}

// One workgroup over pool[2][65536]: thread t owns the bins 256 t .. 256 t + 255 of a region.
__global__ __launch_bounds__(kQThreads) void quantile_pooled_kernel(const unsigned long long *__restrict__ pool, Quantiles q,
                                                                    int n_q, mccnn_eval_quantiles_t *__restrict__ result)
{
    constexpr int kOwn = kPoolBins / kQThreads;
    __shared__ uint64_t wave_total[kQWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int r = 0; r < 2; ++r) {
        mccnn_quantile_region_t *reg = r == 0 ? &result->all : &result->nonocc;
        const unsigned long long *mine = pool + (size_t)r * kPoolBins + (size_t)tid * kOwn;
        uint64_t local = 0;
#pragma unroll 8
        for (int j = 0; j < kOwn; ++j) local += mine[j];
        uint64_t incl = wave_scan(local, lane);
        __syncthreads();                                         // the previous region's totals are consumed
        if (lane == kWave - 1) wave_total[wave] = incl;
        __syncthreads();
        uint64_t n = 0;
#pragma unroll
        for (int w = 0; w < kQWaves; ++w) {
            if (w < wave) incl += wave_total[w];
            n += wave_total[w];
        }
        if (tid == 0) reg->n_scored = n;
        for (int k = 0; k < kQ; ++k) {
            if (k >= n_q || n == 0) {
                if (tid == 0) write_entry(reg, k, 0, k < n_q ? kNaNBits : 0u);
                continue;
            }
            const uint64_t rank = rank_of(q.ppm[k], n);
            uint64_t below = incl - local;
            if (rank >= below && rank < incl) {                  // one thread
                int b = 0;
                for (; b < kOwn - 1; ++b) {
                    const uint64_t c = mine[b];
                    if (rank < below + c) break;
                    below += c;
                }
                write_entry(reg, k, rank, (uint32_t)(tid * kOwn + b) << 16);
            }
        }
    }
}

int check_quantiles(const char *who, const uint32_t *q_ppm, int n_q, Quantiles *q)
{
    MCCNN_REQUIRE(n_q >= 1 && n_q <= kQ, MCCNN_E_INVALID, "%s: n_q=%d, expected 1..%d", who, n_q, kQ);
    for (int k = 0; k < kQ; ++k) {
        q->ppm[k] = k < n_q ? q_ppm[k] : 1000000u;
        MCCNN_REQUIRE(q->ppm[k] >= 1u && q->ppm[k] <= 1000000u, MCCNN_E_INVALID, "%s: q_ppm[%d]=%u, expected 1..1000000", who, k,
                      q->ppm[k]);
    }
    return 0;
}

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace
}  // namespace mccnn

extern "C" size_t mccnn_evaluate_quantiles_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return mccnn::kScratchBytes;
}

extern "C" int mccnn_evaluate_quantiles(const float *disp, const float *gt, const uint8_t *mask, int H, int W,
                                        const uint32_t *q_ppm, int n_q, mccnn_eval_quantiles_t *result, uint64_t *pool,
                                        void *scratch, size_t scratch_bytes, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_evaluate_quantiles";
    MCCNN_REQUIRE(disp && gt && q_ppm && scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(result || pool, MCCNN_E_INVALID, "%s: null pointer: neither result nor pool", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    Quantiles q;
    if (int rc = check_quantiles(who, q_ppm, n_q, &q)) return rc;
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kQMaxPixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, the 32-bit bin counts hold H*W <= %llu", who, H, W, (unsigned long long)kQMaxPixels);
    MCCNN_REQUIRE(scratch_bytes >= kScratchBytes, MCCNN_E_SCRATCH,
                  "%s: scratch of %zu bytes, mccnn_evaluate_quantiles_scratch_bytes(%d, %d) = %zu", who, scratch_bytes, H, W,
                  kScratchBytes);
    MCCNN_REQUIRE(aligned8(scratch) && aligned8(result) && aligned8(pool), MCCNN_E_INVALID,
                  "%s: scratch, result and pool must be 8-byte aligned", who);
    const size_t n = (size_t)H * W;
    const size_t per_group = (size_t)kQThreads * kQTerms;
    const size_t groups = (n + per_group - 1) / per_group;
    const dim3 grid((unsigned)(groups < (size_t)kQMaxGrid ? groups : (size_t)kQMaxGrid)), block(kQThreads);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *pl = reinterpret_cast<unsigned long long *>(pool);
    SelectState *state = static_cast<SelectState *>(scratch);
    if (!result) {
        hipLaunchKernelGGL((quantile_hist_kernel<0, false, true>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                           (uint32_t *)nullptr, pl);
        return check_launch(who);
    }
    const hipError_t e = hipMemsetAsync(hist_of(scratch, 0), 0, kHistBytes, s);
    if (e != hipSuccess) {
        set_error("%s: clearing the histograms: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    if (pool)
        hipLaunchKernelGGL((quantile_hist_kernel<0, true, true>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                           hist_of(scratch, 0), pl);
    else
        hipLaunchKernelGGL((quantile_hist_kernel<0, true, false>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                           hist_of(scratch, 0), pl);
    hipLaunchKernelGGL(quantile_select_kernel, dim3(1), block, 0, s, hist_of(scratch, 0), 0, q, n_q, state, result);
    hipLaunchKernelGGL((quantile_hist_kernel<1, true, false>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                       hist_of(scratch, 1), pl);
    hipLaunchKernelGGL(quantile_select_kernel, dim3(1), block, 0, s, hist_of(scratch, 1), 1, q, n_q, state, result);
    hipLaunchKernelGGL((quantile_hist_kernel<2, true, false>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                       hist_of(scratch, 2), pl);
    hipLaunchKernelGGL(quantile_select_kernel, dim3(1), block, 0, s, hist_of(scratch, 2), 2, q, n_q, state, result);
    hipLaunchKernelGGL((quantile_hist_kernel<3, true, false>), grid, block, 0, s, disp, gt, mask, n, n_q, state,
                       hist_of(scratch, 3), pl);
    hipLaunchKernelGGL(quantile_select_kernel, dim3(1), block, 0, s, hist_of(scratch, 3), 3, q, n_q, state, result);
    return check_launch(who);
}

extern "C" int mccnn_evaluate_quantiles_pooled(const uint64_t *pool, const uint32_t *q_ppm, int n_q,
                                               mccnn_eval_quantiles_t *result, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_evaluate_quantiles_pooled";
    MCCNN_REQUIRE(pool && q_ppm && result, MCCNN_E_INVALID, "%s: null pointer", who);
    Quantiles q;
    if (int rc = check_quantiles(who, q_ppm, n_q, &q)) return rc;
    MCCNN_REQUIRE(aligned8(pool) && aligned8(result), MCCNN_E_INVALID, "%s: pool and result must be 8-byte aligned", who);
    hipLaunchKernelGGL(quantile_pooled_kernel, dim3(1), dim3(kQThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long *>(pool), q, n_q, result);
    return check_launch(who);
}
