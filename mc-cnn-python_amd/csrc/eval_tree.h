// The bit-defined sums of the evaluation entry points (include/mccnn.h: mccnn_evaluate, mccnn_evaluate_kitti), shared by
// csrc/evaluate.hip and csrc/kitti.hip: each has its own per-pixel rule and hands the terms of a chunk to chunk_reduce().
//
// The pixels are cut into chunks of 1024 consecutive indices; the 1024 terms of a chunk (+0.0 for a pixel outside the
// region, invalid or past the end) are reduced by the stride-halving tree
//     for s = 512, 256, ..., 1:  x[j] += x[j + s]  for j < s
// and the chunk partials are added in ascending chunk order from +0.0.  One workgroup of 256 threads per chunk; thread t
// owns the terms t, t + 256, t + 512, t + 768 (coalesced loads), so the levels s = 512 and 256 are (x0 + x2) + (x1 + x3)
// in registers, s = 128 and 64 go through LDS, and s = 32 .. 1 are lane shifts inside the first wave (lane j reads lane
// j + s; float64 addition commutes, so x[j] + x[j+s] has the tree's bits).  The same tree serves sum_abs and sum_sq of both
// regions.  Counts are integers, combined in any order: one ballot + population count per predicate and wave.
//
// Two launches, no atomics on memory:
//   1. a chunk kernel          one workgroup per chunk -> scratch: 4 float64 partials + 20 uint32 counts per chunk
//   2. evaluate_finish_kernel  one workgroup: the partials added in chunk order (staged through LDS 256 chunks at a
//                              time, one thread per sum), the counts added up, `result` overwritten or accumulated into
#pragma once
#include "common.h"

namespace mccnn {
namespace {

constexpr int kChunk = 1024;
constexpr int kThreads = 256;
constexpr int kTerms = kChunk / kThreads;                         // per thread
constexpr int kWaves = kThreads / kWave;
constexpr int kSums = 4;                                          // all.abs, all.sq, nonocc.abs, nonocc.sq
constexpr int kCountsPerRegion = 2 + MCCNN_EVAL_MAX_THRESHOLDS;   // n_valid, n_invalid, n_bad[8]
constexpr int kCounts = 2 * kCountsPerRegion;
constexpr size_t kChunkBytes = kSums * sizeof(double) + kCounts * sizeof(uint32_t);

static_assert(sizeof(mccnn_eval_region_t) == 96 && sizeof(mccnn_eval_t) == 192, "mccnn_eval_t layout");
static_assert(kTerms == 4, "the in-register tree levels are written for four terms per thread");

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// The tail of a chunk kernel: a[r][e], q[r][e] are this thread's terms of region r, c[] its wave's counts (every lane
// of a wave holds the same values).  Called by all 256 threads of the workgroup of chunk `chunk`.
__device__ __forceinline__ void chunk_reduce(const double (&a)[2][kTerms], const double (&q)[2][kTerms],
                                             const uint32_t (&c)[kCounts], size_t chunk, double *__restrict__ partial,
                                             uint32_t *__restrict__ counts)
{
    __shared__ double x[kSums][kThreads];
    __shared__ uint32_t wave_counts[kWaves][kCounts];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    // s = 512, 256: x[t] += x[t+512], x[t+256] += x[t+768]; x[t] += x[t+256]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        x[2 * r][tid] = (a[r][0] + a[r][2]) + (a[r][1] + a[r][3]);
        x[2 * r + 1][tid] = (q[r][0] + q[r][2]) + (q[r][1] + q[r][3]);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kCounts; ++k) wave_counts[wave][k] = c[k];
    }
    __syncthreads();
    if (tid < 128) {
#pragma unroll
        for (int v = 0; v < kSums; ++v) x[v][tid] += x[v][tid + 128];
    }
    __syncthreads();
    if (tid < kWave) {
        double s[kSums];
#pragma unroll
        for (int v = 0; v < kSums; ++v) s[v] = x[v][tid] + x[v][tid + 64];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
            for (int v = 0; v < kSums; ++v) s[v] += __shfl_down(s[v], d, kWave);   // lanes >= d: unused from here on
        }
        if (tid == 0) {
#pragma unroll
            for (int v = 0; v < kSums; ++v) partial[chunk * kSums + v] = s[v];
        }
    }
    if (tid >= kWave && tid < kWave + kCounts) {     // second wave: the four waves' counts
        const int k = tid - kWave;
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += wave_counts[w][k];
        counts[chunk * kCounts + k] = t;
    }
}

// Position of count k (region r, field f) in mccnn_eval_t, in uint64 words.
__device__ __forceinline__ int count_word(int k)
{
    const int r = k / kCountsPerRegion, f = k % kCountsPerRegion;
    return r * (int)(sizeof(mccnn_eval_region_t) / 8) + f;
}

__global__ __launch_bounds__(kThreads) void evaluate_finish_kernel(const double *__restrict__ partial,
                                                                   const uint32_t *__restrict__ counts, size_t nchunks,
                                                                   int n_thr, int accumulate, mccnn_eval_t *__restrict__ result)
{
    __shared__ double stage[kThreads][kSums];
    __shared__ unsigned long long wave_totals[kWaves][kCounts];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

    // counts: any order
    unsigned long long mine[kCounts];
#pragma unroll
    for (int k = 0; k < kCounts; ++k) mine[k] = 0;
    for (size_t ch = tid; ch < nchunks; ch += kThreads) {
#pragma unroll
        for (int k = 0; k < kCounts; ++k) mine[k] += counts[ch * kCounts + k];
    }
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {
        unsigned long long t = mine[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_down(t, d, kWave);
        if (lane == 0) wave_totals[wave][k] = t;
    }

    // sums: ascending chunk order from +0.0, thread v < 4 owns sum v
    double total = 0.0;
    for (size_t c0 = 0; c0 < nchunks; c0 += kThreads) {
        const size_t left = nchunks - c0;
        const int m = left < (size_t)kThreads ? (int)left : kThreads;
        __syncthreads();     // the previous batch is consumed (first pass: wave_totals are written)
        if (tid < m) {
#pragma unroll
            for (int v = 0; v < kSums; ++v) stage[tid][v] = partial[(c0 + tid) * kSums + v];
        }
        __syncthreads();
        if (tid < kSums) {
#pragma unroll 8
            for (int j = 0; j < m; ++j) total += stage[j][tid];
        }
    }
    __syncthreads();         // nchunks >= 1, so this is reached behind the wave_totals in any case

    uint64_t *words = reinterpret_cast<uint64_t *>(result);
    if (tid < kCounts) {
        const int f = tid % kCountsPerRegion;
        const bool used = f < 2 + n_thr;
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += wave_totals[w][tid];
        uint64_t *dst = words + count_word(tid);
        if (!accumulate)
            *dst = used ? t : 0;
        else if (used)
            *dst += t;
    }
    if (tid < kSums) {
        mccnn_eval_region_t *reg = tid < 2 ? &result->all : &result->nonocc;
        double *dst = (tid & 1) ? &reg->sum_sq : &reg->sum_abs;
        *dst = accumulate ? *dst + total : total;
    }
}

// Largest H*W: the chunk index is the workgroup index of the first launch (grid.x).
constexpr uint64_t kMaxChunks = 2147483647ull;
constexpr uint64_t kMaxPixels = kMaxChunks * kChunk;

inline uint64_t chunks_of(int H, int W) { return ((uint64_t)H * (uint64_t)W + kChunk - 1) / kChunk; }

// Bytes of the per-chunk partials and counts of an H x W map, rounded up to 16.
inline size_t chunk_scratch_bytes(int H, int W) { return (size_t)((chunks_of(H, W) * kChunkBytes + 15) & ~(uint64_t)15); }

}  // namespace
}  // namespace mccnn
