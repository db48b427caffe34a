// KITTI 2012 / 2015 on the device (include/mccnn.h: mccnn_kitti_encode_u16, mccnn_kitti_decode_u16,
// mccnn_kitti_interpolate_background, mccnn_evaluate_kitti), after the development kit as remembered; the text in the header is the definition.
//
// A disparity is valid when it is finite and >= 0 (-0.0f is valid) - the rule of mccnn_evaluate.
//
// encode_u16_kernel        one thread per pixel: 0 for an invalid one, else rintf(d * 256) clamped to 1 .. 65535.
//                          6 bytes per pixel.
// decode_u16_kernel        the way back: code / 256 (exact), 0 -> +inf - "unknown" as a ground truth, invalid as an estimate.
// fill_rows_kernel         the kit's interpolateBackground along the rows, without its sequential walk: an invalid pixel
//                          takes the smaller of its nearest valid neighbours to the left and to the right in its row (the
//                          left one on a tie), or the one it has.  One workgroup of 256 threads per row sweeps the row in
//                          segments of 256 pixels, forwards for the left neighbour and backwards for the right one.  Inside
//                          a wave a 64-bit ballot of "valid" and a count of leading (trailing) zeros names the nearest valid
//                          lane at or below (above) a lane, and a lane read fetches its value; every wave leaves its last
//                          (first) valid value in LDS for the waves behind it, and the last valid value of a segment is
//                          carried into the next one in a register.  The forward sweep writes the left neighbour into `out`
//                          (an invalid pixel without one keeps its bits, which are invalid: that is the flag); the backward
//                          sweep reads it back - every pixel is written and read by the same thread - and combines.
//                          12 bytes per pixel read, 4 to 8 written.
// fill_columns_kernel      one thread per column, in place: finds the first valid row from the top and the last from the
//                          bottom, and copies them upwards and downwards.  After the row pass a row is valid or invalid as
//                          a whole, so the scans stop at the first whole valid row: what is read and written is the
//                          invalid margin.
// evaluate_kitti_chunk_kernel   the per-pixel rule of mccnn_evaluate_kitti on 16-bit ground truth, on the tree of
//                          csrc/eval_tree.h; the finish kernel is the one of mccnn_evaluate.  8 to 10 bytes per pixel.
// All of it is launch-bound at KITTI's 1242 x 375 (1.9 MB of float32 per map).
#include <math.h>

#include "eval_tree.h"

namespace mccnn {
namespace {

__device__ __forceinline__ bool valid_disparity(float d) { return isfinite(d) && d >= 0.f; }

__global__ __launch_bounds__(kThreads) void encode_u16_kernel(const float *__restrict__ disp, size_t n,
                                                               uint16_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float d = disp[i];
    uint16_t code = 0;
    if (valid_disparity(d)) {
        const float v = rintf(d * 256.0f);        // round half to even; +inf when the product overflows
        code = v < 1.f ? (uint16_t)1 : v > 65535.f ? (uint16_t)65535 : (uint16_t)v;
    }
    out[i] = code;
}

__global__ __launch_bounds__(kThreads) void decode_u16_kernel(const uint16_t *__restrict__ code, size_t n,
                                                               float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = code[i];
    out[i] = c ? (float)c / 256.0f : INFINITY;
}

// One direction of the row pass.  FORWARD: `near` is the nearest valid value at or left of the pixel; otherwise at or
// right of it.  The LDS slots alternate between segments, so one barrier per segment is enough: a wave can write slot p
// again only behind the barrier of the segment in between, which every wave reaches after its reads of slot p.
template <bool FORWARD>
__device__ __forceinline__ void sweep_row(const float *__restrict__ in, float *__restrict__ out, int W, int nseg,
                                          float (&wave_value)[2][kWaves], int (&wave_has)[2][kWaves], int &slot)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float carry = 0.f;
    bool carry_has = false;
    for (int k = 0; k < nseg; ++k) {
        const int seg = FORWARD ? k : nseg - 1 - k;
        const int w = seg * kThreads + tid;
        const bool inside = w < W;
        const float d = inside ? in[w] : -1.f;
        const bool v = inside && valid_disparity(d);
        const unsigned long long mask = __ballot(v);
        const unsigned long long mine = FORWARD ? mask & (~0ull >> (63 - lane)) : mask & (~0ull << lane);
        bool has = mine != 0;
        const int src = FORWARD ? 63 - __clzll((long long)mine) : __ffsll((long long)mine) - 1;
        float near = __shfl(d, has ? src : lane, kWave);
        const int edge = FORWARD ? 63 - __clzll((long long)mask) : __ffsll((long long)mask) - 1;
        const float edge_value = __shfl(d, mask ? edge : 0, kWave);
        if (lane == 0) {
            wave_value[slot][wave] = edge_value;
            wave_has[slot][wave] = mask != 0;
        }
        __syncthreads();
        if (!has) {
            for (int j = 1; j < kWaves && !has; ++j) {          // the waves before (behind) this one, nearest first
                const int o = FORWARD ? wave - j : wave + j;
                if (o >= 0 && o < kWaves && wave_has[slot][o]) {
                    near = wave_value[slot][o];
                    has = true;
                }
            }
        }
        if (!has && carry_has) {
            near = carry;
            has = true;
        }
        for (int j = 0; j < kWaves; ++j) {                      // the segment's last (first) valid value, if it has one
            const int o = FORWARD ? j : kWaves - 1 - j;
            if (wave_has[slot][o]) {
                carry = wave_value[slot][o];
                carry_has = true;
            }
        }
        slot ^= 1;
        if (!inside) continue;
        if (FORWARD) {
            out[w] = has ? near : d;                            // a valid pixel is its own nearest: copied bit for bit
        } else if (!v && has) {
            const float left = out[w];                          // this thread's own store of the forward sweep
            out[w] = valid_disparity(left) ? (near < left ? near : left) : near;
        }
    }
}

__global__ __launch_bounds__(kThreads) void fill_rows_kernel(const float *__restrict__ disp, int W, float *__restrict__ out)
{
    __shared__ float wave_value[2][kWaves];
    __shared__ int wave_has[2][kWaves];
    const size_t row = (size_t)blockIdx.x * (size_t)W;
    const int nseg = (W + kThreads - 1) / kThreads;
    int slot = 0;
    sweep_row<true>(disp + row, out + row, W, nseg, wave_value, wave_has, slot);
    sweep_row<false>(disp + row, out + row, W, nseg, wave_value, wave_has, slot);
}

__global__ __launch_bounds__(kThreads) void fill_columns_kernel(float *__restrict__ map, int H, int W)
{
    const int w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= W) return;
    float *col = map + w;
    int first = 0;
    while (first < H && !valid_disparity(col[(size_t)first * W])) ++first;
    if (first == H) return;                                     // nothing valid in this column: it stays as it is
    int last = H - 1;
    while (!valid_disparity(col[(size_t)last * W])) --last;     // stops at `first` at the latest
    const float top = col[(size_t)first * W], bottom = col[(size_t)last * W];
    for (int h = 0; h < first; ++h) col[(size_t)h * W] = top;
    for (int h = last + 1; h < H; ++h) col[(size_t)h * W] = bottom;
}

void launch_interpolate_background(const float *disp, int H, int W, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(fill_rows_kernel, dim3((unsigned)H), dim3(kThreads), 0, s, disp, W, out);
    hipLaunchKernelGGL(fill_columns_kernel, dim3((unsigned)cdiv(W, kThreads)), dim3(kThreads), 0, s, out, H, W);
}

struct KittiThresholds {
    float abs[MCCNN_EVAL_MAX_THRESHOLDS], rel[MCCNN_EVAL_MAX_THRESHOLDS];
};

__global__ __launch_bounds__(kThreads) void evaluate_kitti_chunk_kernel(const float *__restrict__ disp,
                                                                         const uint16_t *__restrict__ gt_occ,
                                                                         const uint16_t *__restrict__ gt_noc, size_t n,
                                                                         KittiThresholds thr, int n_thr,
                                                                         double *__restrict__ partial,
                                                                         uint32_t *__restrict__ counts)
{
    const int tid = threadIdx.x;
    const size_t chunk = blockIdx.x;
    const size_t base = chunk * kChunk;

    double a[2][kTerms], q[2][kTerms];
    uint32_t c[kCounts];
#pragma unroll
    for (int k = 0; k < kCounts; ++k) c[k] = 0;
#pragma unroll
    for (int e = 0; e < kTerms; ++e) {
        const size_t i = base + (size_t)e * kThreads + tid;
        const bool inside = i < n;
        const uint32_t occ = inside ? gt_occ[i] : 0u;
        const uint32_t code[2] = {occ, (inside && gt_noc) ? gt_noc[i] : occ};
        const float d = inside ? disp[i] : 0.f;
        const bool invalid = !valid_disparity(d);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool region = code[r] != 0u;
            const float g = (float)code[r] / 256.0f;            // exact
            const float err = fabsf(d - g);
            const bool scored = region && !invalid;
            a[r][e] = scored ? (double)err : 0.0;
            q[r][e] = scored ? (double)err * (double)err : 0.0;
            uint32_t *cr = c + r * kCountsPerRegion;
            cr[0] += wave_count(region);
            cr[1] += wave_count(region && invalid);
#pragma unroll
            for (int k = 0; k < MCCNN_EVAL_MAX_THRESHOLDS; ++k) {
                const float rel = thr.rel[k] * g;               // a float32 product of its own (-ffp-contract=off)
                cr[2 + k] += wave_count(scored && k < n_thr && err > thr.abs[k] && err > rel);
            }
        }
    }
    chunk_reduce(a, q, c, chunk, partial, counts);
}

// Largest H*W of the encode and the decode: one thread per pixel, the workgroup index in grid.x.
constexpr uint64_t kMaxEncodePixels = 2147483647ull * kThreads;

inline size_t map_bytes(int H, int W) { return (size_t)(((uint64_t)H * (uint64_t)W * sizeof(float) + 15) & ~(uint64_t)15); }

}  // namespace
}  // namespace mccnn

extern "C" int mccnn_kitti_encode_u16(const float *disp, int H, int W, uint16_t *out_u16, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_kitti_encode_u16";
    MCCNN_REQUIRE(disp && out_u16, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(disp) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_u16) & 1u) == 0,
                  MCCNN_E_INVALID, "%s: disp must be 4-byte aligned and out_u16 2-byte aligned", who);
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxEncodePixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, the workgroup index holds H*W <= %llu", who, H, W, (unsigned long long)kMaxEncodePixels);
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(encode_u16_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, disp, n, out_u16);
    return check_launch(who);
}

extern "C" int mccnn_kitti_decode_u16(const uint16_t *code_u16, int H, int W, float *out, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_kitti_decode_u16";
    MCCNN_REQUIRE(code_u16 && out, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(code_u16) & 1u) == 0,
                  MCCNN_E_INVALID, "%s: out must be 4-byte aligned and code_u16 2-byte aligned", who);
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxEncodePixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, the workgroup index holds H*W <= %llu", who, H, W, (unsigned long long)kMaxEncodePixels);
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(decode_u16_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, code_u16, n, out);
    return check_launch(who);
}

extern "C" int mccnn_kitti_interpolate_background(const float *disp, int H, int W, float *out, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_kitti_interpolate_background";
    MCCNN_REQUIRE(disp && out, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(out != disp, MCCNN_E_INVALID, "%s: out must not be disp (the row pass reads disp behind its own writes)", who);
    MCCNN_REQUIRE(((reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, MCCNN_E_INVALID,
                  "%s: disp and out must be 4-byte aligned", who);
    launch_interpolate_background(disp, H, W, out, (hipStream_t)stream);
    return check_launch(who);
}

extern "C" size_t mccnn_evaluate_kitti_scratch_bytes(int H, int W, int interpolate)
{
    if (H <= 0 || W <= 0) return 0;
    return mccnn::chunk_scratch_bytes(H, W) + (interpolate ? mccnn::map_bytes(H, W) : 0);
}

extern "C" int mccnn_evaluate_kitti(const float *disp, const uint16_t *gt_occ_u16, const uint16_t *gt_noc_u16, int H, int W,
                                    const float *abs_thr, const float *rel_thr, int n_thr, int interpolate, int accumulate,
                                    mccnn_eval_t *result, void *scratch, size_t scratch_bytes, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_evaluate_kitti";
    MCCNN_REQUIRE(disp && gt_occ_u16 && abs_thr && rel_thr && result && scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(n_thr >= 1 && n_thr <= MCCNN_EVAL_MAX_THRESHOLDS, MCCNN_E_INVALID, "%s: n_thr=%d, expected 1..%d", who, n_thr,
                  MCCNN_EVAL_MAX_THRESHOLDS);
    KittiThresholds thr;
    for (int k = 0; k < MCCNN_EVAL_MAX_THRESHOLDS; ++k) {
        thr.abs[k] = k < n_thr ? abs_thr[k] : INFINITY;
        thr.rel[k] = k < n_thr ? rel_thr[k] : 0.f;
        MCCNN_REQUIRE(!isnan(thr.abs[k]) && !isnan(thr.rel[k]), MCCNN_E_INVALID, "%s: threshold %d is NaN", who, k);
        MCCNN_REQUIRE(thr.abs[k] >= 0.f && thr.rel[k] >= 0.f, MCCNN_E_INVALID, "%s: threshold %d is negative", who, k);
    }
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxPixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, the chunk index holds H*W <= %llu", who, H, W, (unsigned long long)kMaxPixels);
    const size_t need = mccnn_evaluate_kitti_scratch_bytes(H, W, interpolate);
    MCCNN_REQUIRE(scratch_bytes >= need, MCCNN_E_SCRATCH,
                  "%s: scratch of %zu bytes, mccnn_evaluate_kitti_scratch_bytes(%d, %d, %d) = %zu", who, scratch_bytes, H, W,
                  interpolate ? 1 : 0, need);
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0 && (reinterpret_cast<uintptr_t>(result) & 7u) == 0,
                  MCCNN_E_INVALID, "%s: scratch and result must be 8-byte aligned", who);
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(disp) & 3u) == 0 && (reinterpret_cast<uintptr_t>(gt_occ_u16) & 1u) == 0 &&
                      (reinterpret_cast<uintptr_t>(gt_noc_u16) & 1u) == 0,
                  MCCNN_E_INVALID, "%s: disp must be 4-byte aligned and the ground truth 2-byte aligned", who);
    const size_t n = (size_t)H * W;
    const size_t nchunks = (size_t)chunks_of(H, W);
    double *partial = static_cast<double *>(scratch);
    uint32_t *counts = reinterpret_cast<uint32_t *>(partial + nchunks * kSums);
    hipStream_t s = (hipStream_t)stream;
    const float *scored = disp;
    if (interpolate) {       // the filled map lives in scratch, behind the chunk partials; disp is only read
        float *filled = reinterpret_cast<float *>(static_cast<char *>(scratch) + chunk_scratch_bytes(H, W));
        launch_interpolate_background(disp, H, W, filled, s);
        scored = filled;
    }
    hipLaunchKernelGGL(evaluate_kitti_chunk_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, scored, gt_occ_u16, gt_noc_u16,
                       n, thr, n_thr, partial, counts);
    hipLaunchKernelGGL(evaluate_finish_kernel, dim3(1), dim3(kThreads), 0, s, partial, counts, nchunks, n_thr, accumulate ? 1 : 0,
                       result);
    return check_launch(who);
}
