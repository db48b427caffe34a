// a4 cost_volume_aggregation in the reference's summation order (pf:149-163, bit-exact) on pixel-major volumes
// [H][W][Dp] for arms up to 31, i.e. distance thresholds up to 32 - the whole range of the support word's 5-bit arms.
// The design is cbca_hwd.hip's (read its header first): disparities on lanes, the walk over the support region on
// the scalar unit, every region row loaded once into a statically indexed register window and shared by the pixels of
// the wave, each pixel's chain the same flat float32 running sum in the same order.  What changes with the radius:
//
//   * R = 31.  cbca_hwd_kernel's window (G + 2 R slots of VPL floats) would need (5 + 62) x 4 = 268 registers; here a
//     wave owns G = 2 neighbouring pixels of ONE image row (K = 1) and two disparities per lane: 64 slots x 2 = 128
//     window registers, 138 VGPRs in all, no scratch - planned for 3 waves per SIMD.  Wider volumes run as
//     chunks of 128 disparities (blockIdx.z), so there is a single disparities-per-lane variant.
//   * The window masks are 64-bit words derived in the kernel from the arm fields of plane 0 (one shift per pixel
//     and row on the scalar unit); the support buffer keeps its layout and cbca_hwd_kernel's 32-bit mask plane is not
//     read.  With one anchor row per wave the sweep schedule is two compares instead of a bit word.
//   * The input descriptor is rebuilt per region row (a 64-bit scalar add) and spans that row only, so the reach
//     condition is one row, W * Dp * 4 < 2^31, and no load can leave the row it was issued for.
//
// Launch order (XCD bands, column sweep inside a band) and the epilogue discipline (quotients first, then the stores
// behind a scheduling barrier) are cbca_hwd_kernel's.  The last iteration is followed by mccnn_wta_hwd: a wave holds 128
// disparities, so a fused WTA would serve D <= 128 only.
#include "support.h"

namespace mccnn {
namespace hwl {

constexpr int R = 31;                  // longest arm served (distance threshold L <= 32)
constexpr int G = 2;                   // pixels per wave
constexpr int NW = G + 2 * R;          // window slots: columns x0 - R .. x0 + G - 1 + R
constexpr int VPL = 2;                 // disparities per lane
constexpr int kDrop = 0x7ffffff0;      // byte offset past every buffer: the range check drops the access
typedef uint64_t wm_t;                 // window mask: one bit per slot
constexpr wm_t kOne = 1;
static_assert(NW <= 64, "window masks are 64-bit words");

#ifndef CBCA_HWDL_NTS
#define CBCA_HWDL_NTS 2                // aux bits of the result stores (2 = non-temporal)
#endif
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct vf { float x, y; };            // two scalars, not a vector type: built with -fno-slp-vectorize (Makefile), see
                                       // cbca_hwd.hip's Vec::add
__device__ __forceinline__ vf vload(__amdgpu_buffer_rsrc_t rs, int voff, unsigned soff)
{
    const u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
    vf v;
    v.x = __uint_as_float(u.x); v.y = __uint_as_float(u.y);
    return v;
}
__device__ __forceinline__ void vstore(vf v, __amdgpu_buffer_rsrc_t rs, int voff, unsigned soff)
{
    u32x2 u;
    u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y);
    __builtin_amdgcn_raw_buffer_store_b64(u, rs, voff, soff, CBCA_HWDL_NTS);   // 8-byte stores: no data-register hazard
}
__device__ __forceinline__ void vadd(vf &a, const vf &w) { a.x += w.x; a.y += w.y; }

// One arm of pixel J on one region row: elements Z = 1 .. along DIR while the mask has them.  Long arms are what this
// kernel is for, so they are taken four elements per scalar test; the arm's end falls back to single tests.
template <int J, int Z, int DIR>   // DIR = -1: left arm (slots below J + R), +1: right arm
__device__ __forceinline__ void walk_arm(vf &a, const vf (&win)[NW], wm_t m)
{
    if constexpr (Z <= R) {
        if (m & (kOne << (J + R + DIR * Z))) {
            if constexpr (Z + 3 <= R) {
                constexpr wm_t four = DIR > 0 ? ((wm_t)0xF << (J + R + Z)) : ((wm_t)0xF << (J + R - Z - 3));
                if ((~m & four) == 0) {
                    vadd(a, win[J + R + DIR * Z]);
                    vadd(a, win[J + R + DIR * (Z + 1)]);
                    vadd(a, win[J + R + DIR * (Z + 2)]);
                    vadd(a, win[J + R + DIR * (Z + 3)]);
                    walk_arm<J, Z + 4, DIR>(a, win, m);
                } else {                                   // the arm ends within the next three elements
                    vadd(a, win[J + R + DIR * Z]);
                    if (m & (kOne << (J + R + DIR * (Z + 1)))) {
                        vadd(a, win[J + R + DIR * (Z + 1)]);
                        if (m & (kOne << (J + R + DIR * (Z + 2)))) vadd(a, win[J + R + DIR * (Z + 2)]);
                    }
                }
            } else {
                vadd(a, win[J + R + DIR * Z]);
                walk_arm<J, Z + 1, DIR>(a, win, m);
            }
        }
    }
}
// pf:157-161 for pixel J on one region row: self, left 1.., right 1..
template <int J>
__device__ __forceinline__ void walk_rows(vf (&acc)[G], const vf (&win)[NW], const wm_t (&m)[G])
{
    if constexpr (J < G) {
        if (m[J] != 0) {
            vadd(acc[J], win[J + R]);
            if (m[J] != (kOne << (J + R))) {
                walk_arm<J, 1, -1>(acc[J], win, m[J]);
                walk_arm<J, 1, +1>(acc[J], win, m[J]);
            }
        }
        walk_rows<J + 1>(acc, win, m);
    }
}

// Loads the window slots whose bits are set in `u` (the OR of the row's masks): a scalar test per nibble of four
// slots, then per slot.
template <int N>
__device__ __forceinline__ void load_window(vf (&win)[NW], wm_t u, __amdgpu_buffer_rsrc_t rs, int voff, unsigned rowoff,
                                            unsigned pix)
{
    if constexpr (4 * N < NW) {
        if (u & ((wm_t)0xF << (4 * N))) {
            unsigned off = rowoff + (unsigned)(4 * N) * pix;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (4 * N + i < NW) {
                    if (u & (kOne << (4 * N + i))) win[4 * N + i] = vload(rs, voff, off);
                    off += pix;
                }
            }
        }
        load_window<N + 1>(win, u, rs, voff, rowoff, pix);
    }
}

// One launch aggregates up to two volumes of the same shape (left and right view, each with its own support plane).
struct Jobs {
    const float *in[2];
    float *out[2];
    const Support *sup[2];
    int n;
};

// The window mask of the pixel in column x (x0 + j) of a region row, from its support word: one bit per slot its
// horizontal arms cover, the arms clamped to the image so that no slot outside the row is ever asked for.
__device__ __forceinline__ wm_t row_mask(uint32_t w, int j, int x, int W)
{
    const int l = min(arm_left(w), x), r = min(arm_right(w), W - 1 - x);
    return (((wm_t)2 << (l + r)) - 1) << (j + R - l);
}

// grid = (8 * band_rows, ngroups, nchunks * jobs): blockIdx.x & 7 = XCD = band of `band_rows` image rows,
// blockIdx.x >> 3 = row inside the band, blockIdx.y = group of G columns, blockIdx.z = (job, chunk of 64 * VPL
// disparities).  Dispatch order is x fastest, then y: inside its band an XCD sweeps column group by column group.
// A wave visits the rows of its G regions in one descending sweep y0, y0 - 1, .. (self, up 1..) and one ascending
// sweep y0 + 1, .. (down 1..), pf:155's order for every pixel; a pixel sits out the rows beyond its own arm.
__global__ __launch_bounds__(64) void cbca_hwd_long_kernel(const Jobs jobs, int Dp, int H, int W, int nchunks, int band_rows)
{
    const int lane = threadIdx.x & 63;
    const int y0 = (int)(blockIdx.x & 7) * band_rows + (int)(blockIdx.x >> 3);
    if (y0 >= H) return;
    const int x0 = (int)blockIdx.y * G;
    const int job = (int)blockIdx.z / nchunks, chunk = (int)blockIdx.z - job * nchunks;
    const float *const in = job ? jobs.in[1] : jobs.in[0];
    float *const out = job ? jobs.out[1] : jobs.out[0];
    const Support *__restrict__ const sup = job ? jobs.sup[1] : jobs.sup[0];

    const unsigned pix = (unsigned)Dp * 4u;                        // bytes between neighbouring pixels
    const size_t rowf = (size_t)W * Dp;                            // floats per image row
    const int d0 = (chunk * 64 + lane) * VPL;
    const int voff = d0 < Dp ? d0 * 4 : kDrop;                     // lanes past the disparity range: loads 0, stores dropped

    // anchors: vertical arms (plane 0), clamped to the image.  The word of a column past the right edge is read from
    // inside the support buffer (its derived planes follow plane 0) and never used: that pixel joins no row.
    int up[G], dn[G];
    float cnt[G];
    int nd = 1, na = 0;                                            // descending steps y0 .. , ascending steps y0 + 1 ..
    {
        const size_t p0 = (size_t)y0 * W + x0;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const uint32_t aw = sup[p0 + j];
            const bool ok = x0 + j < W;
            up[j] = ok ? min(arm_up(aw), y0) : -1;
            dn[j] = ok ? min(arm_down(aw), H - 1 - y0) : 0;
            cnt[j] = (float)sup_count(aw);
            nd = max(nd, up[j] + 1);
            na = max(na, dn[j]);
        }
    }
    const int nsteps = nd + na;
    auto row_of = [&](int t) { return t < nd ? y0 - t : y0 + 1 + (t - nd); };

    vf acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j].x = acc[j].y = 0.f;        // pf:156 sum starts at 0

    uint32_t nxt[G];
#pragma unroll
    for (int j = 0; j < G; ++j) nxt[j] = sup[(size_t)y0 * W + x0 + j];
    for (int t = 0; t < nsteps; ++t) {
        const int yq = row_of(t);
        wm_t m[G], u = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const bool in_row = t < nd ? t <= up[j] : t - nd < dn[j];
            m[j] = in_row ? row_mask(nxt[j], j, x0 + j, W) : (wm_t)0;
            u |= m[j];
        }
        {   // the next row's arms travel while this row is loaded and summed (past the end: a harmless re-read)
            const size_t pn = (size_t)row_of(min(t + 1, nsteps - 1)) * W + x0;
#pragma unroll
            for (int j = 0; j < G; ++j) nxt[j] = sup[pn + j];
        }
        // this row alone: slot k = column x0 - R + k; the offset wraps below zero for slots left of the image, which
        // no clamped arm reaches
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float *>(in + (size_t)yq * rowf), 0, (int)(rowf * 4), 0x00020000);
        const unsigned rowoff = (unsigned)((x0 - R) * (int)pix);
        vf win[NW];
        load_window<0>(win, u, rs_in, voff, rowoff, pix);
        walk_rows<0>(acc, win, m);
    }
    // Epilogue as in cbca_hwd_kernel: every quotient into registers of its own, then the stores behind a scheduling
    // barrier.  The descriptor ends with the row: the store of a column past the right edge is dropped by its range check.
    vf res[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        res[j].x = acc[j].x / cnt[j];                              // pf:161
        res[j].y = acc[j].y / cnt[j];
    }
    __builtin_amdgcn_sched_barrier(0);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
        out + ((size_t)y0 * W + x0) * Dp, 0, (int)((unsigned)min(G, W - x0) * pix), 0x00020000);
#pragma unroll
    for (int j = 0; j < G; ++j) vstore(res[j], rs_out, voff, (unsigned)j * pix);
}

static int launch(const Jobs &jobs, int D, int H, int W, hipStream_t s, const char *who)
{
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "%s: %d columns x %d disparities exceed a buffer descriptor's reach", who, W, D);
    const int nchunks = cdiv(Dp, 64 * VPL);
    const int band_rows = cdiv(H, 8);
    const int ngroups = cdiv(W, G);
    MCCNN_REQUIRE(ngroups <= 65535 && nchunks * jobs.n <= 65535, MCCNN_E_UNSUPPORTED, "%s: %dx%dx%d exceeds the grid", who,
                  W, H, D);
    const dim3 grid(8 * band_rows, ngroups, nchunks * jobs.n), block(64);
    hipLaunchKernelGGL(cbca_hwd_long_kernel, grid, block, 0, s, jobs, Dp, H, W, nchunks, band_rows);
    return check_launch(who);
}

}  // namespace hwl
}  // namespace mccnn

extern "C" int mccnn_cbca_iter_hwd_long(const float *in_hwd, float *out_hwd, const mccnn_support_t *support, int D, int H,
                                        int W, int L, mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *const who = "mccnn_cbca_iter_hwd_long";
    MCCNN_REQUIRE(in_hwd && out_hwd && support, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(in_hwd != out_hwd, MCCNN_E_INVALID, "%s: in-place aggregation is not defined (ping-pong)", who);
    MCCNN_REQUIRE(D > 0 && H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(L >= 1 && L <= 32, MCCNN_E_UNSUPPORTED, "%s: L=%d outside [1,32] (5-bit arms)", who, L);
    if (const int rc = check_support_record(support, H, W, L, who, true)) return rc;
    const hwl::Jobs jobs = {{in_hwd, nullptr}, {out_hwd, nullptr}, {support, nullptr}, 1};
    return hwl::launch(jobs, D, H, W, (hipStream_t)stream, who);
}

extern "C" int mccnn_cbca_iter_hwd_long_pair(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                                             const float *in_right, float *out_right,
                                             const mccnn_support_t *support_right, int D, int H, int W, int L,
                                             mccnn_stream_t stream)
{
    using namespace mccnn;
    const char *const who = "mccnn_cbca_iter_hwd_long_pair";
    MCCNN_REQUIRE(in_left && out_left && support_left && in_right && out_right && support_right, MCCNN_E_INVALID,
                  "%s: null pointer", who);
    MCCNN_REQUIRE(in_left != out_left && in_right != out_right && out_left != out_right && in_left != out_right &&
                      in_right != out_left,
                  MCCNN_E_INVALID, "%s: outputs must not alias an input or each other", who);
    MCCNN_REQUIRE(D > 0 && H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(L >= 1 && L <= 32, MCCNN_E_UNSUPPORTED, "%s: L=%d outside [1,32] (5-bit arms)", who, L);
    int rc = check_support_record(support_left, H, W, L, who, true);
    if (rc) return rc;
    rc = check_support_record(support_right, H, W, L, who, true);
    if (rc) return rc;
    const hwl::Jobs jobs = {{in_left, in_right}, {out_left, out_right}, {support_left, support_right}, 2};
    return hwl::launch(jobs, D, H, W, (hipStream_t)stream, who);
}
