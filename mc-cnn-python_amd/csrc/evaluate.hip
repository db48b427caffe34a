// Device-side evaluation of a disparity map against ground truth (include/mccnn.h: mccnn_evaluate), after the
// Middlebury SDK's evaldisp as remembered; the text in the header is the definition.
//
// Per pixel i = h*W + w, for each of the two regions (all: gt finite; nonocc: also mask == 255, or all without a mask):
//   n_valid += 1;  disp not finite or disp < 0: n_invalid += 1, nothing else;
//   otherwise err = fabsf(disp - gt) (float32), n_bad[k] += err > thr[k], and the pixel's terms are
//   a = (double)err, q = (double)err * (double)err (exact in float64).
//
// The sums are defined to the bit; the tree, the two-launch scheme and the finish kernel are in csrc/eval_tree.h, which
// mccnn_evaluate_kitti (csrc/kitti.hip) shares.  Here: evaluate_chunk_kernel, one workgroup per chunk of 1024 pixels.
// 3.4 MB for a 750 x 500 map: launch-bound.
#include <math.h>

#include "eval_tree.h"

namespace mccnn {
namespace {

struct Thresholds {
    float t[MCCNN_EVAL_MAX_THRESHOLDS];
};

__global__ __launch_bounds__(kThreads) void evaluate_chunk_kernel(const float *__restrict__ disp, const float *__restrict__ gt,
                                                                  const uint8_t *__restrict__ mask, size_t n, Thresholds thr,
                                                                  int n_thr, double *__restrict__ partial,
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
        const float g = inside ? gt[i] : INFINITY;
        const float d = inside ? disp[i] : 0.f;
        const uint32_t m = (inside && mask) ? mask[i] : 255u;
        const bool in_all = inside && isfinite(g);
        const bool region[2] = {in_all, in_all && m == 255u};
        const bool invalid = !isfinite(d) || d < 0.f;
        const float err = fabsf(d - g);
        const double ea = (double)err, eq = (double)err * (double)err;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool scored = region[r] && !invalid;
            a[r][e] = scored ? ea : 0.0;
            q[r][e] = scored ? eq : 0.0;
            uint32_t *cr = c + r * kCountsPerRegion;
            cr[0] += wave_count(region[r]);
            cr[1] += wave_count(region[r] && invalid);
#pragma unroll
            for (int k = 0; k < MCCNN_EVAL_MAX_THRESHOLDS; ++k) cr[2 + k] += wave_count(scored && k < n_thr && err > thr.t[k]);
        }
    }
    chunk_reduce(a, q, c, chunk, partial, counts);
}

}  // namespace
}  // namespace mccnn

extern "C" size_t mccnn_evaluate_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return mccnn::chunk_scratch_bytes(H, W);
}

extern "C" int mccnn_evaluate(const float *disp, const float *gt, const uint8_t *mask, int H, int W, const float *thresholds,
                              int n_thr, int accumulate, mccnn_eval_t *result, void *scratch, size_t scratch_bytes,
                              mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *who = "mccnn_evaluate";
    MCCNN_REQUIRE(disp && gt && thresholds && result && scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(n_thr >= 1 && n_thr <= MCCNN_EVAL_MAX_THRESHOLDS, MCCNN_E_INVALID, "%s: n_thr=%d, expected 1..%d", who, n_thr,
                  MCCNN_EVAL_MAX_THRESHOLDS);
    Thresholds thr;
    for (int k = 0; k < MCCNN_EVAL_MAX_THRESHOLDS; ++k) {
        thr.t[k] = k < n_thr ? thresholds[k] : INFINITY;
        MCCNN_REQUIRE(!isnan(thr.t[k]), MCCNN_E_INVALID, "%s: threshold %d is NaN", who, k);
    }
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxPixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, the chunk index holds H*W <= %llu", who, H, W, (unsigned long long)kMaxPixels);
    MCCNN_REQUIRE(scratch_bytes >= mccnn_evaluate_scratch_bytes(H, W), MCCNN_E_SCRATCH,
                  "%s: scratch of %zu bytes, mccnn_evaluate_scratch_bytes(%d, %d) = %zu", who, scratch_bytes, H, W,
                  mccnn_evaluate_scratch_bytes(H, W));
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0 && (reinterpret_cast<uintptr_t>(result) & 7u) == 0,
                  MCCNN_E_INVALID, "%s: scratch and result must be 8-byte aligned", who);
    const size_t n = (size_t)H * W;
    const size_t nchunks = (size_t)chunks_of(H, W);
    double *partial = static_cast<double *>(scratch);
    uint32_t *counts = reinterpret_cast<uint32_t *>(partial + nchunks * kSums);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(evaluate_chunk_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, disp, gt, mask, n, thr, n_thr, partial,
                       counts);
    hipLaunchKernelGGL(evaluate_finish_kernel, dim3(1), dim3(kThreads), 0, s, partial, counts, nchunks, n_thr, accumulate ? 1 : 0,
                       result);
    return check_launch(who);
}
