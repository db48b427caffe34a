// Device-side ingest: the decoded bytes of a PNG ([H][W][C] uint8, C = 1, 3 or 4) -> the standardised float32 image the
// conv stack reads, bit-identical to what match.py computes on the host:
//     g = util.read_gray(p).astype(np.float32);  (g - np.mean(g, axis=(0,1))) / np.std(g, axis=(0,1))
// float32 throughout, un-fused (-ffp-contract=off), correctly rounded division and square root:
//     mean = S(g) / n,  x = g - mean,  var = S(x * x) / n,  std = sqrt(var),  out = (g - mean) / std,  n = float(H * W).
//
// S is NumPy's summation order on a C-contiguous float32 array (2.x, reduction buffer of 8192 elements):
//   - the flat array is cut into consecutive chunks of 8192 elements, the last one shorter;
//   - a chunk c of m elements is summed by the pairwise routine P:
//       m < 8:    0 + c[0] + c[1] + ... in order
//       m <= 128: eight accumulators r[k] = c[k], r[k] += c[i + k] for i = 8, 16, ... < m - m % 8, then
//                 ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the m % 8 tail added in order
//       else:     m2 = m / 2; m2 -= m2 % 8;  P(c[:m2]) + P(c[m2:])
//   - the chunk sums are added left to right: ((0 + P(c0)) + P(c1)) + P(c2) ...
// A full chunk is a balanced tree over 64 leaves of 128 elements: one workgroup per chunk, the chunk in LDS, one leaf per
// lane of the first wave, six adjacent-pair combines across the lanes.  A ragged chunk (the last one) takes the general
// recursion level by level, one thread per node of the tree: split downwards, sum the leaves, combine upwards.
//
// Three launches per image (or per pair: blockIdx.y is the view), all on a grid of one workgroup per chunk:
//   1. ingest_sum_kernel    P(g chunk)                      -> sums[0][chunk]
//   2. ingest_sqsum_kernel  mean from sums[0]; P(x*x chunk)  -> sums[1][chunk]
//   3. ingest_store_kernel  mean, std from sums; out = (g - mean) / std
// The left-to-right pass over the chunk sums (46 for a 750x500 image) is repeated by thread 0 of every workgroup that
// needs it.  Bytes per pixel: 3 C read (L2-resident after the first launch), 4 written.
#include "common.h"

namespace mccnn {
namespace {

constexpr int kChunk = 8192;                       // NumPy's reduction buffer, in elements
constexpr int kLeaf = 128;                         // P's unrolled block
constexpr int kThreads = 256;
constexpr int kLdsFloats = kChunk + kChunk / kLeaf;

struct IngestViews {
    const uint8_t *image[2];
    float *out[2];
};

// LDS position of chunk element j: one pad word per 128 elements, so that the 64 lanes that walk the 64 leaves of a full
// chunk in step (stride 128 elements) fall on different banks.
__device__ __forceinline__ int lds_pos(int j) { return j + (j >> 7); }

// libpng's rgb_to_gray as OpenCV sets it up (util.read_gray): 15-bit weights, truncated.
__device__ __forceinline__ float gray_of(uint32_t r, uint32_t g, uint32_t b)
{
    return (float)((r * 9797u + g * 19234u + b * 3737u) >> 15);
}

// Grey values of the 4 pixels p .. p + 3 (4 C bytes from a 4-byte aligned address: C dword loads).
template <int C>
__device__ __forceinline__ void gray4_aligned(const uint8_t *__restrict__ img, size_t p, float g[4])
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(img + p * C);
    uint32_t w[C];
#pragma unroll
    for (int k = 0; k < C; ++k) w[k] = src[k];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        auto byte = [&](int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; };
        if (C == 1)
            g[q] = (float)byte(q);
        else
            g[q] = gray_of(byte(q * C), byte(q * C + 1), byte(q * C + 2));
    }
}

template <int C>
__device__ __forceinline__ float gray1(const uint8_t *__restrict__ img, size_t p)
{
    const uint8_t *s = img + p * C;
    if (C == 1) return (float)s[0];
    return gray_of(s[0], s[1], s[2]);
}

// f(j, g) for every element j < m of the chunk that starts at pixel e0.
template <int C, typename F>
__device__ __forceinline__ void for_each_gray(const uint8_t *__restrict__ img, size_t e0, int m, int tid, F f)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(img) + e0 * C) & 3u) == 0;
    const int quads = aligned ? (m >> 2) : 0;
    for (int q = tid; q < quads; q += kThreads) {
        float g[4];
        gray4_aligned<C>(img, e0 + 4 * (size_t)q, g);
#pragma unroll
        for (int k = 0; k < 4; ++k) f(4 * q + k, g[k]);
    }
    for (int j = 4 * quads + tid; j < m; j += kThreads) f(j, gray1<C>(img, e0 + j));
}

// P on m <= 128 elements of the chunk in LDS, from element `off` on.
__device__ __forceinline__ float leaf_sum(const float *c, int off, int m)
{
    if (m < 8) {
        float res = 0.f;
        for (int i = 0; i < m; ++i) res += c[lds_pos(off + i)];
        return res;
    }
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = c[lds_pos(off + k)];
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += c[lds_pos(off + i + k)];
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < m; ++i) res += c[lds_pos(off + i)];
    return res;
}

// P's recursion on a ragged chunk (m < 8192), level by level.  The tree has at most 8 levels (a part is 64 .. 128 elements
// long when it stops splitting, and a level-6 part of a chunk below 8192 is at most 142): it is laid out as a heap of 255
// nodes, node 1 the root, node n's parts at 2n and 2n + 1, one thread per node.  Node word: off | len << 13, len 0 = no
// such node.
constexpr int kTreeLevels = 8;
struct TreeLds {
    uint32_t node[1 << kTreeLevels];
    float val[1 << kTreeLevels];
};

// P(chunk of m elements in c); the result is valid in thread 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ float chunk_sum(const float *c, int m, int tid, TreeLds &t)
{
    __syncthreads();   // the chunk is in LDS
    if (m == kChunk) {
        float s = 0.f;
        if (tid < kWave) {
            s = leaf_sum(c, tid * kLeaf, kLeaf);
            // adjacent pairs, then pairs of pairs ...: float addition commutes, so the butterfly leaves the balanced
            // tree's sum in every lane
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) s += __shfl_xor(s, d, kWave);
        }
        return s;
    }
    static_assert(kThreads == (1 << kTreeLevels), "one thread per heap node");
    const int level = tid > 0 ? 31 - __clz(tid) : -1;   // of node `tid`
    if (tid == 1) t.node[1] = (uint32_t)m << 13;
    for (int l = 0; l + 1 < kTreeLevels; ++l) {           // split downwards
        __syncthreads();
        if (level == l) {
            const uint32_t e = t.node[tid];
            const int off = e & 8191, len = e >> 13;
            uint32_t left = 0, right = 0;
            if (len > kLeaf) {
                int m2 = len / 2;
                m2 -= m2 % 8;
                left = (uint32_t)off | ((uint32_t)m2 << 13);
                right = (uint32_t)(off + m2) | ((uint32_t)(len - m2) << 13);
            }
            t.node[2 * tid] = left;
            t.node[2 * tid + 1] = right;
        }
    }
    __syncthreads();
    const uint32_t e = tid > 0 ? t.node[tid] : 0u;
    const int len = e >> 13;
    if (len > 0 && len <= kLeaf) t.val[tid] = leaf_sum(c, e & 8191, len);
    for (int l = kTreeLevels - 2; l >= 0; --l) {          // combine upwards
        __syncthreads();
        if (level == l && len > kLeaf) t.val[tid] = t.val[2 * tid] + t.val[2 * tid + 1];
    }
    __syncthreads();
    return t.val[1];
}

// The chunk sums added left to right.
__device__ __forceinline__ float sum_left_to_right(const float *__restrict__ sums, int nchunks)
{
    float s = 0.f;
    for (int i = 0; i < nchunks; ++i) s += sums[i];
    return s;
}

__device__ __forceinline__ int chunk_len(size_t n, int chunk)
{
    const size_t left = n - (size_t)chunk * kChunk;
    return left < (size_t)kChunk ? (int)left : kChunk;
}

template <int C>
__global__ __launch_bounds__(kThreads) void ingest_sum_kernel(IngestViews v, size_t n, int nchunks, float *__restrict__ sums)
{
    __shared__ float c[kLdsFloats];
    __shared__ TreeLds t;
    const int tid = threadIdx.x, chunk = blockIdx.x, view = blockIdx.y;
    const int m = chunk_len(n, chunk);
    for_each_gray<C>(v.image[view], (size_t)chunk * kChunk, m, tid, [&](int j, float g) { c[lds_pos(j)] = g; });
    const float s = chunk_sum(c, m, tid, t);
    if (tid == 0) sums[(size_t)view * 2 * nchunks + chunk] = s;
}

template <int C>
__global__ __launch_bounds__(kThreads) void ingest_sqsum_kernel(IngestViews v, size_t n, int nchunks, float *__restrict__ sums)
{
    __shared__ float c[kLdsFloats];
    __shared__ TreeLds t;
    __shared__ float mean_s;
    const int tid = threadIdx.x, chunk = blockIdx.x, view = blockIdx.y;
    float *mine = sums + (size_t)view * 2 * nchunks;
    if (tid == 0) mean_s = sum_left_to_right(mine, nchunks) / (float)n;
    __syncthreads();
    const float mean = mean_s;
    const int m = chunk_len(n, chunk);
    for_each_gray<C>(v.image[view], (size_t)chunk * kChunk, m, tid, [&](int j, float g) {
        const float x = g - mean;
        c[lds_pos(j)] = x * x;
    });
    const float s = chunk_sum(c, m, tid, t);
    if (tid == 0) mine[nchunks + chunk] = s;
}

template <int C>
__global__ __launch_bounds__(kThreads) void ingest_store_kernel(IngestViews v, size_t n, int nchunks,
                                                                const float *__restrict__ sums)
{
    __shared__ float stat[2];
    const int tid = threadIdx.x, chunk = blockIdx.x, view = blockIdx.y;
    const float *mine = sums + (size_t)view * 2 * nchunks;
    if (tid == 0) {
        stat[0] = sum_left_to_right(mine, nchunks) / (float)n;
        stat[1] = sqrtf(sum_left_to_right(mine + nchunks, nchunks) / (float)n);
    }
    __syncthreads();
    const float mean = stat[0], sd = stat[1];
    const size_t e0 = (size_t)chunk * kChunk;
    float *__restrict__ out = v.out[view] + e0;
    for_each_gray<C>(v.image[view], e0, chunk_len(n, chunk), tid, [&](int j, float g) { out[j] = (g - mean) / sd; });
}

template <int C>
int launch(const IngestViews &v, int views, size_t n, int nchunks, float *sums, hipStream_t stream, const char *who)
{
    const dim3 grid(nchunks, views), block(kThreads);
    hipLaunchKernelGGL(ingest_sum_kernel<C>, grid, block, 0, stream, v, n, nchunks, sums);
    hipLaunchKernelGGL(ingest_sqsum_kernel<C>, grid, block, 0, stream, v, n, nchunks, sums);
    hipLaunchKernelGGL(ingest_store_kernel<C>, grid, block, 0, stream, v, n, nchunks, sums);
    return check_launch(who);
}

size_t chunks_of(int H, int W) { return ((size_t)H * W + kChunk - 1) / kChunk; }

int ingest(const IngestViews &v, int views, int H, int W, int C, void *scratch, size_t scratch_bytes, hipStream_t stream,
           const char *who)
{
    for (int i = 0; i < views; ++i)
        MCCNN_REQUIRE(v.image[i] && v.out[i], MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(C == 1 || C == 3 || C == 4, MCCNN_E_INVALID, "%s: C=%d, expected 1 (grey), 3 (RGB) or 4 (RGBA)", who, C);
    MCCNN_REQUIRE(scratch_bytes >= mccnn_ingest_scratch_bytes(H, W), MCCNN_E_SCRATCH,
                  "%s: scratch of %zu bytes, mccnn_ingest_scratch_bytes(%d, %d) = %zu", who, scratch_bytes, H, W,
                  mccnn_ingest_scratch_bytes(H, W));
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 3u) == 0, MCCNN_E_INVALID, "%s: scratch must be 4-byte aligned", who);
    for (int i = 0; i < views; ++i)
        MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(v.out[i]) & 3u) == 0, MCCNN_E_INVALID, "%s: out must be 4-byte aligned", who);
    const size_t n = (size_t)H * W;
    const int nchunks = (int)chunks_of(H, W);
    float *sums = static_cast<float *>(scratch);
    if (C == 1) return launch<1>(v, views, n, nchunks, sums, stream, who);
    if (C == 3) return launch<3>(v, views, n, nchunks, sums, stream, who);
    return launch<4>(v, views, n, nchunks, sums, stream, who);
}

}  // namespace
}  // namespace mccnn

// Two views x (chunk sums of g, chunk sums of x*x), one float per chunk each; a single image uses the first half.
extern "C" size_t mccnn_ingest_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return (mccnn::chunks_of(H, W) * 4 * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" int mccnn_ingest_u8(const uint8_t *image_u8, int H, int W, int C, float *out, void *scratch, size_t scratch_bytes,
                               mccnn_stream_t stream)
{
    mccnn::IngestViews v = {{image_u8, nullptr}, {out, nullptr}};
    return mccnn::ingest(v, 1, H, W, C, scratch, scratch_bytes, (hipStream_t)stream, "mccnn_ingest_u8");
}

extern "C" int mccnn_ingest_u8_pair(const uint8_t *left_u8, const uint8_t *right_u8, int H, int W, int C, float *out_left,
                                    float *out_right, void *scratch, size_t scratch_bytes, mccnn_stream_t stream)
{
    mccnn::IngestViews v = {{left_u8, right_u8}, {out_left, out_right}};
    return mccnn::ingest(v, 2, H, W, C, scratch, scratch_bytes, (hipStream_t)stream, "mccnn_ingest_u8_pair");
}
