// Metric outputs of a disparity map (include/mccnn.h has the binding definitions): the depth plane - one streaming
// launch - and the ordered point cloud, a stream compaction in four launches whose count and sizes depend on H and W
// alone: no read-back, no atomics, nothing that waits for another workgroup.
//   1 count   counts[b] = the kept pixels among block b's 1024 consecutive pixels (ballot + popcount).
//   2 scan    every workgroup turns 1024 block counts into their exclusive prefix sums, in place, and writes their sum
//             to totals[g].
//   3 top     ONE workgroup turns the totals into their exclusive prefix sums (1024 at a time, a carry in registers:
//             H*W <= 2^31 - 1 leaves at most 2048 of them) and writes n_points.
//   4 write   block b recomputes its pixels, ranks the kept ones - totals[b / 1024] + counts[b] + the waves in front +
//             the lanes in front (mbcnt of the ballot) - and stores one 16-byte record each.
// A level of the scan is a launch of its own: the stream orders them.  The rank of a pixel is a sum of counts, so the
// order and the bytes are a function of the map alone.  A wave takes 4 x 64 consecutive pixels and a workgroup's four
// waves 1024, so the raster order is wave-major inside a block and one barrier per block is all the exchange there is.
// Launches 1 and 4 evaluate the same keep() on the same bits.
#include "common.h"

namespace mccnn {
namespace reproject {

constexpr uint64_t kMaxPixels = 0x7FFFFFFFull;   // the pixel index and every count fit 32 bits
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSteps = 4;                        // a wave's 4 x 64 consecutive pixels
constexpr unsigned kBlock = kThreads * kSteps;   // pixels per compaction block
constexpr unsigned kLevel = kThreads * 4;        // block counts per scan workgroup: four per thread

struct Camera {
    float fx, fy, cx, cy, fb, doffs, max_depth;
};

// Z = fb / (d + doffs) where d is finite and the denominator positive, +inf elsewhere (NaN fails both compares).
__device__ __forceinline__ float depth_of(float d, float fb, float doffs)
{
    const float den = d + doffs;
    const bool has = fabsf(d) < __builtin_huge_valf() && den > 0.0f;
    return has ? fb / den : __builtin_huge_valf();
}

__device__ __forceinline__ bool keep(float z, float max_depth) { return z < __builtin_huge_valf() && z <= max_depth; }

__global__ __launch_bounds__(kThreads) void depth_kernel(const float *__restrict__ map, size_t N, float fb, float doffs,
                                                         float *__restrict__ depth)
{
    const size_t n = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    depth[n] = depth_of(map[n], fb, doffs);
}

// Pixel `step` of this lane in block b: wave-major, so that a wave's ballots are in raster order.
__device__ __forceinline__ unsigned pixel_of(unsigned b, int wv, int step, int lane)
{
    return b * kBlock + (unsigned)(wv * (64 * kSteps) + step * 64 + lane);
}

__global__ __launch_bounds__(kThreads) void count_kernel(const float *__restrict__ map, unsigned N, Camera c,
                                                         unsigned *__restrict__ counts)
{
    __shared__ unsigned s_wave[kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const unsigned p = pixel_of(blockIdx.x, wv, i, lane);
        const bool k = p < N && keep(depth_of(map[p < N ? p : 0], c.fb, c.doffs), c.max_depth);
        n += (unsigned)__builtin_popcountll(__ballot(k));
    }
    if (lane == 0) s_wave[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// The exclusive prefix sum of `v` over the workgroup's threads, and the workgroup's sum.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *s_wave, unsigned &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const unsigned t = s_wave[w];
        if (w < wv) before += t;
        total += t;
    }
    __syncthreads();        // s_wave is free for the next call
    return before + inc - v;
}

// v[first .. first + kLevel) (below n) -> their exclusive prefix sums plus `carry`, in place; returns their sum.
__device__ __forceinline__ unsigned scan_level(unsigned *v, unsigned first, unsigned n, unsigned carry, unsigned *s_wave)
{
    const unsigned i0 = first + threadIdx.x * 4u;
    unsigned a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = i0 + k < n ? v[i0 + k] : 0u;
    unsigned total;
    unsigned run = carry + block_scan(a[0] + a[1] + a[2] + a[3], s_wave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) v[i0 + k] = run;
        run += a[k];
    }
    return total;
}

__global__ __launch_bounds__(kThreads) void scan_kernel(unsigned *counts, unsigned n, unsigned *__restrict__ totals)
{
    __shared__ unsigned s_wave[kWaves];
    const unsigned total = scan_level(counts, blockIdx.x * kLevel, n, 0u, s_wave);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void top_kernel(unsigned *totals, unsigned n, uint32_t *__restrict__ n_points)
{
    __shared__ unsigned s_wave[kWaves];
    unsigned carry = 0;
    for (unsigned first = 0; first < n; first += kLevel) carry += scan_level(totals, first, n, carry, s_wave);
    if (threadIdx.x == 0) *n_points = carry;
}

__global__ __launch_bounds__(kThreads) void write_kernel(const float *__restrict__ map, unsigned N, unsigned W, Camera c,
                                                         const unsigned *__restrict__ counts,
                                                         const unsigned *__restrict__ totals, uint4 *__restrict__ points)
{
    __shared__ unsigned s_wave[kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float z[kSteps];
    unsigned long long m[kSteps];
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const unsigned p = pixel_of(blockIdx.x, wv, i, lane);
        z[i] = p < N ? depth_of(map[p], c.fb, c.doffs) : __builtin_huge_valf();
        m[i] = __ballot(keep(z[i], c.max_depth));
        n += (unsigned)__builtin_popcountll(m[i]);
    }
    if (lane == 0) s_wave[wv] = n;
    __syncthreads();
    size_t at = (size_t)totals[blockIdx.x / kLevel] + counts[blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wv) at += s_wave[w];
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        if (m[i] >> lane & 1ull) {
            const unsigned p = pixel_of(blockIdx.x, wv, i, lane);
            const unsigned h = p / W, w = p - h * W;
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m[i] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m[i], 0u));
            const float x = (((float)w - c.cx) * z[i]) / c.fx;      // sub, mul, div: never fused (-ffp-contract=off)
            const float y = (((float)h - c.cy) * z[i]) / c.fy;
            points[at + rank] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z[i]), p);
        }
        at += (unsigned)__builtin_popcountll(m[i]);
    }
}

static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

static bool positive(float v) { return v > 0.0f && v < __builtin_huge_valf(); }
static bool finite(float v) { return v - v == 0.0f; }

}  // namespace reproject
}  // namespace mccnn

extern "C" int mccnn_depth(const float *map, int H, int W, float fb, float doffs, float *depth, mccnn_stream_t stream)
{
    using namespace mccnn;
    using namespace mccnn::reproject;
    const char *who = "mccnn_depth";
    MCCNN_REQUIRE(map && depth, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(positive(fb), MCCNN_E_INVALID, "%s: fb=%g, expected a finite value > 0", who, (double)fb);
    MCCNN_REQUIRE(finite(doffs), MCCNN_E_INVALID, "%s: doffs=%g, expected a finite value", who, (double)doffs);
    const size_t N = (size_t)H * W, plane = N * sizeof(float);
    MCCNN_REQUIRE(!overlaps(depth, plane, map, plane), MCCNN_E_INVALID, "%s: depth overlaps map", who);
    MCCNN_REQUIRE((N + kThreads - 1) / kThreads <= 0x7FFFFFFFull, MCCNN_E_UNSUPPORTED, "%s: %d x %d pixels exceed grid.x", who,
                  H, W);
    hipLaunchKernelGGL(depth_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       map, N, fb, doffs, depth);
    return check_launch(who);
}

extern "C" size_t mccnn_points_scratch_bytes(int H, int W)
{
    using namespace mccnn::reproject;
    if (H <= 0 || W <= 0 || (uint64_t)H * (uint64_t)W > kMaxPixels) return 0;
    const size_t blocks = ((size_t)H * W + kBlock - 1) / kBlock, groups = (blocks + kLevel - 1) / kLevel;
    return ((blocks + groups) * sizeof(uint32_t) + 15) & ~(size_t)15;     // counts[blocks], totals[groups]
}

extern "C" int mccnn_reproject_points(const float *map, int H, int W, float fx, float fy, float cx, float cy, float fb,
                                      float doffs, float max_depth, float *points, uint32_t *n_points, void *scratch,
                                      size_t scratch_bytes, mccnn_stream_t stream)
{
    using namespace mccnn;
    using namespace mccnn::reproject;
    const char *who = "mccnn_reproject_points";
    MCCNN_REQUIRE(map && points && n_points && scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(positive(fx), MCCNN_E_INVALID, "%s: fx=%g, expected a finite value > 0", who, (double)fx);
    MCCNN_REQUIRE(positive(fy), MCCNN_E_INVALID, "%s: fy=%g, expected a finite value > 0", who, (double)fy);
    MCCNN_REQUIRE(positive(fb), MCCNN_E_INVALID, "%s: fb=%g, expected a finite value > 0", who, (double)fb);
    MCCNN_REQUIRE(finite(cx) && finite(cy), MCCNN_E_INVALID, "%s: cx=%g, cy=%g, expected finite values", who, (double)cx,
                  (double)cy);
    MCCNN_REQUIRE(finite(doffs), MCCNN_E_INVALID, "%s: doffs=%g, expected a finite value", who, (double)doffs);
    MCCNN_REQUIRE(max_depth == max_depth, MCCNN_E_INVALID, "%s: max_depth is NaN", who);
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxPixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, a pixel index holds H*W <= %llu", who, H, W, (unsigned long long)kMaxPixels);
    const size_t need = mccnn_points_scratch_bytes(H, W);
    MCCNN_REQUIRE(scratch_bytes >= need, MCCNN_E_SCRATCH, "%s: scratch of %zu bytes, mccnn_points_scratch_bytes(%d, %d) = %zu",
                  who, scratch_bytes, H, W, need);
    MCCNN_REQUIRE(aligned16(scratch), MCCNN_E_SCRATCH, "%s: scratch must be 16-byte aligned", who);
    MCCNN_REQUIRE(aligned16(points), MCCNN_E_INVALID, "%s: points must be 16-byte aligned", who);
    const size_t plane = (size_t)H * W * sizeof(float), cloud = plane * 4;
    MCCNN_REQUIRE(!overlaps(points, cloud, map, plane) && !overlaps(n_points, 4, map, plane), MCCNN_E_INVALID,
                  "%s: output overlaps map", who);
    MCCNN_REQUIRE(!overlaps(points, cloud, n_points, 4), MCCNN_E_INVALID, "%s: n_points overlaps points", who);
    MCCNN_REQUIRE(!overlaps(scratch, need, map, plane) && !overlaps(scratch, need, points, cloud) &&
                      !overlaps(scratch, need, n_points, 4),
                  MCCNN_E_INVALID, "%s: scratch overlaps a buffer", who);
    const unsigned N = (unsigned)((size_t)H * W);
    const unsigned blocks = (N + kBlock - 1) / kBlock, groups = (blocks + kLevel - 1) / kLevel;
    unsigned *counts = static_cast<unsigned *>(scratch), *totals = counts + blocks;
    const Camera c = {fx, fy, cx, cy, fb, doffs, max_depth};
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kThreads);
    hipLaunchKernelGGL(count_kernel, dim3(blocks), block, 0, s, map, N, c, counts);
    hipLaunchKernelGGL(scan_kernel, dim3(groups), block, 0, s, counts, blocks, totals);
    hipLaunchKernelGGL(top_kernel, dim3(1), block, 0, s, totals, groups, n_points);
    hipLaunchKernelGGL(write_kernel, dim3(blocks), block, 0, s, map, N, (unsigned)W, c, counts, totals,
                       reinterpret_cast<uint4 *>(points));
    return check_launch(who);
}
