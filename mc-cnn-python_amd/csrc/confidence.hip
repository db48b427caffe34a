// Confidence measures of the left disparity (include/mccnn.h has the binding definitions): one streaming read of the
// final aggregated left volume, 4 B/voxel, whichever measures are asked for.  MSM, MMN and CUR need the volume alone,
// LRC the right winner-take-all map besides.  Every value is one to three un-fused float32 operations on costs that
// are fetched by index, so the two layouts agree bit for bit.
#include "common.h"
#include "wave_reduce.h"

namespace mccnn {
namespace conf {

constexpr unsigned kAll = MCCNN_CONF_MSM | MCCNN_CONF_MMN | MCCNN_CONF_CUR | MCCNN_CONF_LRC;

// One more cost of the scan: b1 / bd the lowest so far with its (first) index, b2 the lowest of all the others.  A value
// equal to b1 at a later index becomes b2; NaN and +inf never enter (both compares are strict and start from +inf).
// A deposed b1 takes second place unconditionally: it is <= b2, and where the two are equal it has the earlier index.
__device__ __forceinline__ void scan(float v, int d, float &b1, int &bd, float &b2)
{
    const bool first = v < b1;
    b2 = first ? b1 : (v < b2 ? v : b2);
    if (first) { b1 = v; bd = d; }
}

// The planes of one pixel from its winner d1 (< 0: none), the runner-up's cost c2 and the pixel's costs c[d * stride].
// MIRROR: the right view's measures (mccnn_confidence_right*): the volume is the right one, `dr` the LEFT disparity map,
// and LRC looks up column w + d1.
template <bool MIRROR>
__device__ __forceinline__ void write_planes(const float *__restrict__ c, size_t stride, int d1, float c2, int D, int W,
                                             long n, long N, const float *__restrict__ dr, unsigned measures,
                                             float *__restrict__ out)
{
    const float ninf = -__builtin_huge_valf();
    float msm = ninf, mmn = ninf, cur = ninf, lrc = ninf;
    if (d1 >= 0) {
        // (c1 feeds three of the four measures and c2 is in a register: MSM and MMN are computed unguarded - one cached
        // load, two operations - while CUR and LRC, which load more, run only when asked for)
        const float c1 = c[(size_t)d1 * stride];
        msm = -c1;
        mmn = c2 - c1;
        if (measures & MCCNN_CONF_CUR) {
            const float cm = c[(size_t)(d1 >= 1 ? d1 - 1 : d1 + 1) * stride];
            const float cp = c[(size_t)(d1 <= D - 2 ? d1 + 1 : d1 - 1) * stride];
            const float t = 2.0f * c1;
            const float u = cp - t;
            cur = u + cm;
        }
        if (measures & MCCNN_CONF_LRC) {
            const int w = (int)(n % W);
            const int x = MIRROR ? w + d1 : w - d1;
            if (MIRROR ? x <= W - 1 : x >= 0) {
                const float r = dr[MIRROR ? n + d1 : n - d1];       // row h, column x
                if (r >= 0.0f && r != __builtin_huge_valf()) lrc = -fabsf((float)d1 - r);
            }
        }
    }
    float *o = out + n;
    if (measures & MCCNN_CONF_MSM) { *o = msm; o += N; }
    if (measures & MCCNN_CONF_MMN) { *o = mmn; o += N; }
    if (measures & MCCNN_CONF_CUR) { *o = cur; o += N; }
    if (measures & MCCNN_CONF_LRC) { *o = lrc; }
}

// ---- pixel-major [H][W][Dp] -----------------------------------------------------------------------------------------
// wta_hwd_kernel's shape: one pixel per wave step, one float4 per lane and 256-disparity group, 8 pixels (8 KiB of
// loads) in flight per wave.  Three wave reductions per pixel: the minimum, the lowest index among its holders (d1), and
// the minimum of what is left - the owner of d1 offers its second value, every other lane its lowest.  A minimum's BITS
// are not unique for zero alone (-0.0 == +0.0): a runner-up that compares equal to zero is looked up again, first
// index first, as the definition's scan meets it.  c[d1], c[d1 +- 1] and the right map are fetched by the storing lane.
template <bool MIRROR>
__global__ __launch_bounds__(256) void confidence_hwd_kernel(const float *__restrict__ vol, const float *__restrict__ dr,
                                                             int D, int Dp, int W, long N, unsigned measures,
                                                             float *__restrict__ out, int per_wave)
{
    constexpr int PF = 8;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long n0 = wave * per_wave, n1 = min(n0 + per_wave, N);
    if (n0 >= N) return;
    const int ng = (Dp + 255) / 256;
    for (long nb = n0; nb < n1; nb += PF) {
        float b1[PF], b2[PF];
        int bd[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            b1[k] = b2[k] = __builtin_huge_valf();
            bd[k] = -1;
        }
        for (int g = 0; g < ng; ++g) {
            const int d = g * 256 + lane * 4;
            float4 v[PF];
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const long n = min(nb + k, n1 - 1);
                v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (d < Dp) v[k] = *reinterpret_cast<const float4 *>(vol + (size_t)n * Dp + d);
            }
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                if (d + 0 < D) scan(v[k].x, d + 0, b1[k], bd[k], b2[k]);
                if (d + 1 < D) scan(v[k].y, d + 1, b1[k], bd[k], b2[k]);
                if (d + 2 < D) scan(v[k].z, d + 2, b1[k], bd[k], b2[k]);
                if (d + 3 < D) scan(v[k].w, d + 3, b1[k], bd[k], b2[k]);
            }
        }
        int d1 = -1, i2 = -1;       // of pixel nb + lane: the winner, and where to fetch a runner-up that is a zero
        float c2 = 0.f;
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const float m = wave_min_f(b1[k]);
            const int cand = (b1[k] == m && bd[k] >= 0) ? bd[k] : 0x7fffffff;
            const int idx = wave_min_i(cand);
            const float m2 = wave_min_f(bd[k] == idx ? b2[k] : b1[k]);
            int z = -1;
            if (m2 == 0.f) {                                // wave-uniform
                const float *p = vol + (size_t)min(nb + k, n1 - 1) * Dp;
                int first = 0x7fffffff;
                for (int g = ng - 1; g >= 0; --g) {
                    const int d = g * 256 + lane * 4;
                    if (d >= Dp) continue;
                    const float4 q = *reinterpret_cast<const float4 *>(p + d);
                    if (d + 3 < D && d + 3 != idx && q.w == 0.f) first = d + 3;
                    if (d + 2 < D && d + 2 != idx && q.z == 0.f) first = d + 2;
                    if (d + 1 < D && d + 1 != idx && q.y == 0.f) first = d + 1;
                    if (d + 0 < D && d + 0 != idx && q.x == 0.f) first = d + 0;
                }
                z = wave_min_i(first);
            }
            if (lane == k) {
                d1 = idx == 0x7fffffff ? -1 : idx;
                c2 = m2;
                i2 = z;
            }
        }
        if (lane < PF && nb + lane < n1) {
            const long n = nb + lane;
            const float *p = vol + (size_t)n * Dp;
            if (i2 >= 0) c2 = p[i2];
            write_planes<MIRROR>(p, 1, d1, c2, D, W, n, N, dr, measures, out);
        }
    }
}

// ---- plane-major [D][H][W] ------------------------------------------------------------------------------------------
// wta_kernel's shape (post.hip): one thread per pixel, adjacent lanes on adjacent columns.  The scan is sequential in d,
// so among equal costs the earlier index takes each place, zeros included.
template <bool MIRROR>
__global__ __launch_bounds__(256) void confidence_kernel(const float *__restrict__ vol, const float *__restrict__ dr,
                                                         int D, int W, long N, unsigned measures,
                                                         float *__restrict__ out)
{
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float b1 = __builtin_huge_valf(), b2 = __builtin_huge_valf();
    int bd = -1;
    const float *p = vol + n;
    int d = 0;
    for (; d + 4 <= D; d += 4) {
        const float v0 = p[(size_t)(d + 0) * N], v1 = p[(size_t)(d + 1) * N], v2 = p[(size_t)(d + 2) * N],
                    v3 = p[(size_t)(d + 3) * N];
        scan(v0, d + 0, b1, bd, b2);
        scan(v1, d + 1, b1, bd, b2);
        scan(v2, d + 2, b1, bd, b2);
        scan(v3, d + 3, b1, bd, b2);
    }
    for (; d < D; ++d) scan(p[(size_t)d * N], d, b1, bd, b2);
    write_planes<MIRROR>(p, (size_t)N, bd, b2, D, W, n, N, dr, measures, out);
}

static int validate(const char *who, const float *vol, const float *dr, int D, int H, int W, unsigned measures,
                    const float *out, const char *other)
{
    MCCNN_REQUIRE(vol && out, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(D >= 2, MCCNN_E_INVALID, "%s: D=%d, the measures need at least two disparities", who, D);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(measures != 0 && (measures & ~kAll) == 0, MCCNN_E_INVALID,
                  "%s: measures=0x%x is not a non-empty set of MCCNN_CONF_* bits", who, measures);
    MCCNN_REQUIRE(dr || !(measures & MCCNN_CONF_LRC), MCCNN_E_INVALID, "%s: MCCNN_CONF_LRC without %s", who, other);
    if (dr) {
        const size_t plane = (size_t)H * W * sizeof(float);
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + plane * (size_t)__builtin_popcount(measures);
        const uintptr_t r0 = (uintptr_t)dr, r1 = r0 + plane;
        MCCNN_REQUIRE(o1 <= r0 || r1 <= o0, MCCNN_E_INVALID, "%s: out overlaps %s", who, other);
    }
    return 0;
}

// One launcher per layout.  MIRROR: the right view's measures; `other`: the name of the other view's map in refusals.
template <bool MIRROR>
static int launch_hwd(const float *vol_hwd, const float *dr, int D, int H, int W, unsigned measures, float *out,
                      hipStream_t s, const char *who, const char *other)
{
    if (const int rc = validate(who, vol_hwd, dr, D, H, W, measures, out, other)) return rc;
    MCCNN_REQUIRE(D <= 1024, MCCNN_E_UNSUPPORTED, "%s: D=%d above 1024", who, D);
    const long N = (long)H * W;
    const int per_wave = 64;   // pixels per wave: 8 rounds of 8
    const long waves = (N + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(confidence_hwd_kernel<MIRROR>, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, vol_hwd, dr, D,
                       mccnn_hwd_pitch(D), W, N, measures, out, per_wave);
    return check_launch(who);
}

template <bool MIRROR>
static int launch_dhw(const float *vol_dhw, const float *dr, int D, int H, int W, unsigned measures, float *out,
                      hipStream_t s, const char *who, const char *other)
{
    if (const int rc = validate(who, vol_dhw, dr, D, H, W, measures, out, other)) return rc;
    const long N = (long)H * W;
    hipLaunchKernelGGL(confidence_kernel<MIRROR>, dim3(cdiv(N, 256)), dim3(256), 0, s, vol_dhw, dr, D, W, N, measures, out);
    return check_launch(who);
}

}  // namespace conf
}  // namespace mccnn

extern "C" int mccnn_confidence_hwd(const float *vol_hwd, const float *disp_right, int D, int H, int W, unsigned measures,
                                    float *out, mccnn_stream_t stream)
{
    return mccnn::conf::launch_hwd<false>(vol_hwd, disp_right, D, H, W, measures, out, (hipStream_t)stream,
                                          "mccnn_confidence_hwd", "disp_right");
}

extern "C" int mccnn_confidence(const float *vol_dhw, const float *disp_right, int D, int H, int W, unsigned measures,
                                float *out, mccnn_stream_t stream)
{
    return mccnn::conf::launch_dhw<false>(vol_dhw, disp_right, D, H, W, measures, out, (hipStream_t)stream,
                                          "mccnn_confidence", "disp_right");
}

extern "C" int mccnn_confidence_right_hwd(const float *vol_right_hwd, const float *disp_left, int D, int H, int W,
                                          unsigned measures, float *out, mccnn_stream_t stream)
{
    return mccnn::conf::launch_hwd<true>(vol_right_hwd, disp_left, D, H, W, measures, out, (hipStream_t)stream,
                                         "mccnn_confidence_right_hwd", "disp_left");
}

extern "C" int mccnn_confidence_right(const float *vol_right_dhw, const float *disp_left, int D, int H, int W,
                                      unsigned measures, float *out, mccnn_stream_t stream)
{
    return mccnn::conf::launch_dhw<true>(vol_right_dhw, disp_left, D, H, W, measures, out, (hipStream_t)stream,
                                         "mccnn_confidence_right", "disp_left");
}
