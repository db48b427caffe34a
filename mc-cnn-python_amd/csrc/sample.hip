// Training patches cut on the device: N sample records -> N patches of ps x ps float32, gathered from a pool of
// standardised images of different sizes that lives in HBM (datagenerator.DevicePatchSampler).  A record names an image
// of the pool, a centre (cy, cx) in it, the 2 x 2 matrix m that maps patch offsets to image offsets, and a gain and a
// bias; every output pixel is one bilinear tap group of that affine warp, zero outside the image (the reference cuts
// from images zero-padded by (ps - 1) / 2, datagenerator.py:141-153; the pool holds them unpadded).
//
// The arithmetic is float32, every operation rounded on its own (-ffp-contract=off) and written in this order, so that
// tests/patch_sampler_reference.py restates it bit for bit.  For output pixel (i, j), c = (ps - 1) / 2, u = j - c,
// v = i - c:
//     x  = cx + ((m[0] * u) + (m[1] * v))        y  = cy + ((m[2] * u) + (m[3] * v))
//     x0 = floorf(x), fx = x - x0                y0 = floorf(y), fy = y - y0
//     tap(yf, xf) = I[(int)yf][(int)xf] if 0 <= yf <= H - 1 and 0 <= xf <= W - 1 (compared as floats, before any
//                   conversion: a centre of +-1e30 reads nothing), else +0.0f
//     row(yy) = tap(yy, x0)                                         if fx == 0   (the second tap is not read)
//             = (tap(yy, x0) * (1 - fx)) + (tap(yy, x0 + 1) * fx)   otherwise
//     val     = row(y0)                                             if fy == 0
//             = (row(y0) * (1 - fy)) + (row(y0 + 1) * fy)           otherwise
//     out     = val                                                 if gain == 1 and bias == 0
//             = (val * gain) + bias                                 otherwise
// The == 0 rules make an identity record (integer centre, m = identity, gain 1, bias 0) a plain copy: the bits of
// ImageDataGenerator._cut, a pixel that is -0.0 included.
//
// One workgroup per patch (a grid-stride loop over the patches: N is never a grid limit): the patch index comes from
// blockIdx, so the record and its image-table row are wave-uniform loads.  At training sizes (384 patches of 121
// pixels, images resident in L2) the launch is bound by its latency, not by bandwidth.
#include <math.h>

#include "common.h"

namespace mccnn {
namespace {

constexpr int kMaxPatch = 31;
constexpr int kMaxBlocks = 1 << 20;     // x 256 threads: well inside a launch's 2^32 work-items

__device__ __forceinline__ float tap(const float *__restrict__ img, float yf, float xf, float hmax, float wmax, int W)
{
    if (yf >= 0.f && yf <= hmax && xf >= 0.f && xf <= wmax) return img[(size_t)(int)yf * W + (int)xf];
    return 0.f;
}

__device__ __forceinline__ float tap_row(const float *__restrict__ img, float yy, float x0, float fx, float hmax, float wmax,
                                         int W)
{
    const float a = tap(img, yy, x0, hmax, wmax, W);
    if (fx == 0.f) return a;
    const float b = tap(img, yy, x0 + 1.f, hmax, wmax, W);
    const float wa = 1.f - fx;
    const float pa = a * wa;
    const float pb = b * fx;
    return pa + pb;
}

__global__ __launch_bounds__(256) void sample_patches_kernel(const float *__restrict__ pool,
                                                             const mccnn_sample_image_t *__restrict__ images,
                                                             const mccnn_sample_t *__restrict__ records, int N, int ps,
                                                             float *__restrict__ out)
{
    const int area = ps * ps;
    const float c = (float)((ps - 1) / 2);
    for (long long n = blockIdx.x; n < N; n += gridDim.x) {      // 64 bits: n + gridDim.x may pass 2^31
        const mccnn_sample_t r = records[n];
        const mccnn_sample_image_t im = images[r.image];
        const float *__restrict__ img = pool + im.offset;
        const float hmax = (float)(im.H - 1), wmax = (float)(im.W - 1);
        const bool plain = r.gain == 1.f && r.bias == 0.f;
        float *__restrict__ dst = out + (size_t)n * area;
        for (int p = threadIdx.x; p < area; p += blockDim.x) {
            const int i = p / ps, j = p - i * ps;
            const float u = (float)j - c, v = (float)i - c;
            const float xu = r.m[0] * u, xv = r.m[1] * v;
            const float xo = xu + xv;
            const float x = r.cx + xo;
            const float yu = r.m[2] * u, yv = r.m[3] * v;
            const float yo = yu + yv;
            const float y = r.cy + yo;
            const float x0 = floorf(x), y0 = floorf(y);
            const float fx = x - x0, fy = y - y0;
            float val = tap_row(img, y0, x0, fx, hmax, wmax, im.W);
            if (fy != 0.f) {
                const float below = tap_row(img, y0 + 1.f, x0, fx, hmax, wmax, im.W);
                const float wa = 1.f - fy;
                const float pa = val * wa;
                const float pb = below * fy;
                val = pa + pb;
            }
            if (!plain) {
                const float scaled = val * r.gain;
                val = scaled + r.bias;
            }
            dst[p] = val;
        }
    }
}

}  // namespace
}  // namespace mccnn

extern "C" int mccnn_sample_patches(const float *pool, const mccnn_sample_image_t *images, int n_images,
                                    const mccnn_sample_t *records, int N, int ps, float *out, mccnn_stream_t stream)
{
    const char *who = "mccnn_sample_patches";
    MCCNN_REQUIRE(pool && images && records && out, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(N >= 1 && n_images >= 1, MCCNN_E_INVALID, "%s: N=%d, n_images=%d, expected at least 1 of each", who, N,
                  n_images);
    MCCNN_REQUIRE(ps >= 1 && (ps & 1), MCCNN_E_INVALID, "%s: ps=%d, expected a positive odd patch side", who, ps);
    MCCNN_REQUIRE(ps <= mccnn::kMaxPatch, MCCNN_E_UNSUPPORTED, "%s: ps=%d, patches of up to %d x %d are supported", who, ps,
                  mccnn::kMaxPatch, mccnn::kMaxPatch);
    const int area = ps * ps;
    const int threads = area <= 64 ? 64 : area <= 128 ? 128 : 256;
    const int blocks = N < mccnn::kMaxBlocks ? N : mccnn::kMaxBlocks;
    hipLaunchKernelGGL(mccnn::sample_patches_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, pool, images,
                       records, N, ps, out);
    return mccnn::check_launch(who);
}
