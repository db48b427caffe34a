// a2  compute_cost_volume (/root/reference/src/process_functional.py:78-113) on gfx950.
//
//   lcv[d,h,w] = -<fl[h,w,:], fr[h,w-d,:]>            w >= d          (pf:87-91, 111)
//   lcv[d,h,w] = mean(lcv[d,h,w+1..w+3])               w <  d, right-to-left recurrence   (pf:94-95)
//   rcv[d,h,w] = lcv[d,h,w+d]                          w <  W-d        (pf:103-104)
//   rcv[d,h,w] = mean(rcv[d,h,w-3..w-1])               w >= W-d, left-to-right recurrence (pf:105-106)
//
// The score matrix of one image row, S[w,w'] = <fl[w], fr[w']>, is a banded product (0 <= w-w' < D); every
// entry feeds lcv[d,h,w] and rcv[d,h,w'] (d = w-w'), both contiguous in w for fixed d, so a workgroup that owns
// 64 columns x 64 disparities of one row writes 256-B runs into both volumes.  Bound: HBM writes (8 B/voxel for
// 128 flop/voxel).  The recurrences run on the already negated values: rounding is sign-symmetric, so
// -((0 - x1 - x2 - x3) / 3) on them has the bits of the reference's fill-then-negate, the sign of an exactly-zero sum
// included (round 6: a plain 0 + x1 + x2 + x3 gave +0.0 there where the reference has -0.0).
//
// MCCNN_CV_EXACT  : VALU kernel that reproduces NumPy's float32 pairwise summation of the 64 products
//                   (8 running sums, fixed combine tree - numpy loops_utils pairwise_sum) bit for bit.
// MCCNN_CV_MFMA   : the 64-channel contraction on the matrix cores: every operand as two f16 numbers (x * 2^10 = hi + lo),
//                   three v_mfma_f32_32x32x16_f16 products per 16 channels, float32 accumulation; within 2e-6 of the
//                   float64 dot product on unit-norm features (measured: 3.6e-7 at most, see the kernel); NaN features
//                   propagate as they do in the exact mode.
#include "common.h"

namespace mccnn {

constexpr int CV_TW = 64;   // output columns per workgroup
constexpr int CV_DT = 64;   // disparities per workgroup
constexpr int CV_C = 64;    // feature channels (NET num_conv_feature_maps)
#ifndef CVM_WAVES_PER_SIMD
#define CVM_WAVES_PER_SIMD 6
#endif
constexpr int CV_LD = 68;   // padded LDS row (floats): 16-B slot index = (row + c4) mod 16 -> conflict-free b128

// PIXEL_MAJOR: the volumes are written "HWD" [H][W][Dp] (the layout the whole bit-exact variant works on) instead of
// [D][H][W]: the 64 x 64 scores of the tile go through LDS (over the left-feature tile, which lives in registers by
// then) - a left-volume pixel receives its 64 disparities as one 256-byte run, a right-volume pixel x = w - d receives
// the anti-diagonal of the tile that belongs to it (up to 64 disparities, one dword per lane).  Entries with w < d
// (left) and x >= W - d (right) are left to cost_volume_fill_hwd_kernel.
template <bool PIXEL_MAJOR>
__global__ __launch_bounds__(256) void cost_volume_exact_kernel(const float *__restrict__ fl,
                                                                const float *__restrict__ fr, int H, int W, int D,
                                                                float *__restrict__ lcv, float *__restrict__ rcv, int Dp)
{
    __shared__ __attribute__((aligned(16))) float sR[(CV_TW + CV_DT - 1) * CV_LD];
    __shared__ __attribute__((aligned(16))) float sL[CV_TW * CV_LD];
    const int w0 = blockIdx.x * CV_TW, h = blockIdx.y, d0 = blockIdx.z * CV_DT;
    if (w0 + CV_TW - 1 < d0) return;  // every (w, d) of this tile has w < d: border fill handles it
    const int tid = threadIdx.x;
    const size_t rowbase = (size_t)h * W;
    for (int i = tid; i < CV_TW * 16; i += 256) {
        const int px = i >> 4, c4 = i & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (w0 + px < W) v = *reinterpret_cast<const float4 *>(fl + (rowbase + w0 + px) * CV_C + c4 * 4);
        *reinterpret_cast<float4 *>(&sL[px * CV_LD + c4 * 4]) = v;
    }
    const int xr0 = w0 - d0 - (CV_DT - 1);  // right-image column held in sR row 0
    for (int i = tid; i < (CV_TW + CV_DT - 1) * 16; i += 256) {
        const int r = i >> 4, c4 = i & 15;
        const int x = xr0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x >= 0 && x < W) v = *reinterpret_cast<const float4 *>(fr + (rowbase + x) * CV_C + c4 * 4);
        *reinterpret_cast<float4 *>(&sR[r * CV_LD + c4 * 4]) = v;
    }
    __syncthreads();

    const int wl = tid & 63, dq = tid >> 6;  // dq is wave-uniform: each wave owns 16 disparities
    const int w = w0 + wl;
    float a[CV_C];
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
        const float4 v = *reinterpret_cast<const float4 *>(&sL[wl * CV_LD + c4 * 4]);
        a[c4 * 4 + 0] = v.x; a[c4 * 4 + 1] = v.y; a[c4 * 4 + 2] = v.z; a[c4 * 4 + 3] = v.w;
    }
    const size_t plane = (size_t)H * W;
    constexpr int TP = 65;              // pitch of the score tile (PIXEL_MAJOR)
    float *const sT = sL;               // every thread holds its left features in registers from here on
    if (PIXEL_MAJOR) __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int d = d0 + dq * 16 + k;
        if (d >= D) break;
        const int r = wl + (CV_DT - 1) - (dq * 16 + k);  // sR row of right column w - d
        if (w < W && w >= d) {
            const float *b = &sR[r * CV_LD];
            float acc[8];
            // numpy pairwise_sum, n = 64: r[j] = p[j]; r[j] += p[8i+j]; ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 b0 = *reinterpret_cast<const float4 *>(b + i * 8);
                const float4 b1 = *reinterpret_cast<const float4 *>(b + i * 8 + 4);
                const float p0 = a[i * 8 + 0] * b0.x, p1 = a[i * 8 + 1] * b0.y, p2 = a[i * 8 + 2] * b0.z,
                            p3 = a[i * 8 + 3] * b0.w, p4 = a[i * 8 + 4] * b1.x, p5 = a[i * 8 + 5] * b1.y,
                            p6 = a[i * 8 + 6] * b1.z, p7 = a[i * 8 + 7] * b1.w;
                if (i == 0) {
                    acc[0] = p0; acc[1] = p1; acc[2] = p2; acc[3] = p3;
                    acc[4] = p4; acc[5] = p5; acc[6] = p6; acc[7] = p7;
                } else {
                    acc[0] += p0; acc[1] += p1; acc[2] += p2; acc[3] += p3;
                    acc[4] += p4; acc[5] += p5; acc[6] += p6; acc[7] += p7;
                }
            }
            float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
            s = 0.f + s;  // np.sum adds the pairwise result to the identity
            s = -1.f * s;
            if (PIXEL_MAJOR) {
                sT[wl * TP + dq * 16 + k] = s;
            } else {
                lcv[(size_t)d * plane + rowbase + w] = s;
                rcv[(size_t)d * plane + rowbase + (w - d)] = s;
            }
        }
    }
    if (PIXEL_MAJOR) {
        __syncthreads();
        const int nd = min(CV_DT, D - d0);           // disparities of this tile that exist
        // left volume: pixel w0 + px, disparities d0 .. d0 + nd - 1 (those with d <= w), 64 lanes = 64 disparities
        const int dl = tid & 63;
        for (int px = tid >> 6; px < CV_TW; px += 4) {
            const int ww = w0 + px, d = d0 + dl;
            if (ww < W && dl < nd && ww >= d) lcv[(rowbase + ww) * (size_t)Dp + d] = sT[px * TP + dl];
        }
        // right volume: pixel x = w - d; its entries of this tile are (w = x + d, d), d0 <= d < d0 + nd
        for (int xi = tid >> 6; xi < CV_TW + CV_DT - 1; xi += 4) {
            const int x = xr0 + xi, d = d0 + dl, px = x + d - w0;      // tile row of w = x + d
            if (x >= 0 && dl < nd && px >= 0 && px < CV_TW && w0 + px < W)
                rcv[(rowbase + x) * (size_t)Dp + d] = sT[px * TP + dl];
        }
    }
}

// ---- bit-exact products for the pixel-major volumes, two scores per LDS row (round 4) ---------------------------------
// cost_volume_exact_kernel<true> is bound by its LDS reads: every score fetches the 64 right-image features of its own
// (w, d) - 256 bytes - out of LDS.  But S(w, d + 1) needs the row of right pixel w - d - 1, which is exactly the row
// lane w - 1 has just fetched for S(w - 1, d): here every lane fetches ONE row per pair of disparities and multiplies
// it twice - with its own left features for d, and, read across the lane boundary by the DPP operand modifier
// (wave_shr:1: lane l reads lane l - 1's register, no extra instruction), for d + 1.  Half the LDS bytes per score; the
// arithmetic and its order per score are unchanged (NumPy's float32 pairwise sum of the 64 rounded products, pf:87-91):
// bit-identical.  Lane 0 has no left neighbour: it is a ghost lane that carries the pixel in front of the tile (the
// last pixel of the tile to the left, which computes that pixel's scores itself), so a tile is 63 pixels wide.  The
// compute is unconditional - a lane's rows must exist for its neighbour - and only the hand-over to the score tile is
// predicated.
constexpr int CVP_TW = 63;   // new pixels per tile (lanes 1 .. 63)
#ifndef CVP_ABL
#define CVP_ABL 0            // timing-only ablations (wrong results): 1 no products, 2 no volume stores
#endif
// (an ablated part stays in the code, behind a condition no real call meets, so that registers and LDS do not change)
__device__ __forceinline__ bool cvp_never(int D) { return D == 12345; }
#ifndef CVP_NT
#define CVP_NT 1             // A/B: the volumes' 16-byte stores carry the non-temporal hint (1) or not (0)
#endif
typedef float cv_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void cvp_store16(char *dst, cv_f4 v)
{
#if CVP_NT
    __builtin_nontemporal_store(v, reinterpret_cast<cv_f4 *>(dst));
#else
    *reinterpret_cast<cv_f4 *>(dst) = v;
#endif
}
__global__ __launch_bounds__(256, 3) void cost_volume_exact_pairs_kernel(const float *__restrict__ fl,
                                                                         const float *__restrict__ fr, int H, int W, int D,
                                                                         float *__restrict__ lcv, float *__restrict__ rcv,
                                                                         int Dp)
{
    // A workgroup owns 63 new pixels of one image row and walks ALL their disparity tiles: the left features stay in
    // registers, and the right-image rows live in a ring of 128 LDS rows indexed by (column & 127) - a tile of 64
    // disparities needs the 127 columns w0 - d0 - 63 .. w0 - d0 + 63, of which the next tile reuses 63: only 64 new
    // rows are fetched per tile (into registers before the tile's products, into the ring behind them).
    constexpr int RING = 128;
    __shared__ __attribute__((aligned(16))) float sR[RING * CV_LD];
    __shared__ __attribute__((aligned(16))) float sL[CV_TW * CV_LD];
    const int w0 = (int)blockIdx.x * CVP_TW - 1, h = blockIdx.y;   // lane 0: pixel w0 (ghost)
    const int tid = threadIdx.x;
    const size_t rowbase = (size_t)h * W;
    // Staging: all of a thread's 4 + 8 loads are issued before the first is waited for (a[] is not live yet, so the
    // twelve float4 fit), and every load is unconditional, so that the compiler's count of loads in flight stays exact.
    // A column outside the image is fetched from the clamped address and kept as it comes: a score S(w, d) is stored
    // only for 0 <= w - d and w < W, so neither a left pixel nor a right column outside the image ever reaches a
    // stored score (the neighbour's row a lane multiplies for d + 1 is column w - d - 1, inside whenever w >= d + 1).
    {
        cv_f4 pl[4], pr[8];   // (the compiler's own vector type: an array of float4 structs copied from memory to memory
                               // is kept in scratch)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256, x = w0 + (i >> 4), c4 = i & 15;
            pl[q] = *reinterpret_cast<const cv_f4 *>(fl + (rowbase + min(max(x, 0), W - 1)) * CV_C + c4 * 4);
        }
        // the first tile's columns w0 - 63 .. w0 + 63
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + q * 256, x = w0 - (CV_DT - 1) + (i >> 4), c4 = i & 15;
            pr[q] = *reinterpret_cast<const cv_f4 *>(fr + (rowbase + min(max(x, 0), W - 1)) * CV_C + c4 * 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256, px = i >> 4, c4 = i & 15;
            *reinterpret_cast<cv_f4 *>(&sL[px * CV_LD + c4 * 4]) = pl[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + q * 256, x = w0 - (CV_DT - 1) + (i >> 4), c4 = i & 15;
            // (the last sixteen threads fill a 128th row, column w0 + 64: its ring slot is the one of column w0 - 64,
            // which no product of the first tile reads and the first tile's prefetch overwrites)
            *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + c4 * 4]) = pr[q];
        }
    }
    __syncthreads();

    const int wl = tid & 63, dq = tid >> 6;  // dq is wave-uniform: each wave owns 16 disparities = 8 pairs of a tile
    const int w = w0 + wl;
    float a[CV_C];
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
        const float4 v = *reinterpret_cast<const float4 *>(&sL[wl * CV_LD + c4 * 4]);
        a[c4 * 4 + 0] = v.x; a[c4 * 4 + 1] = v.y; a[c4 * 4 + 2] = v.z; a[c4 * 4 + 3] = v.w;
    }
    constexpr int TP = CV_LD;           // pitch of the score tile: a multiple of four, so a pixel's disparities leave as float4
    float *const sT = sL;               // every thread holds its left features in registers from here on
    // Both volumes leave as 16-byte stores: 16 lanes x four disparities = one pixel's 64 disparities of a tile, four
    // pixels per wave instruction (a quarter of the store instructions of the one-float-per-lane form: the store phase
    // is bound by their count).  A thread owns 4 quads of the left and 8 of the right volume per tile, at the same
    // places of the score tile in every tile, and classifies each once per tile: a FULL quad (all four entries exist)
    // is one 16-byte store - per volume, all LDS reads first (unconditional, clamped row), then the stores back to
    // back under their predicates; no load is in flight there that a store could be made to wait for, so a wave's
    // stores of one tile retire under its products of the next.  A quad that straddles an edge (w = d, the last
    // disparities when D is no multiple of 4, the image border, the ends of an anti-diagonal) is RAGGED and goes out
    // float by float in a pass of its own behind the full ones.  What decides the class does not change from tile to
    // tile except the quad's first disparity d, so it is one comparison of d with a limit worked out here:
    //   left,  pixel ww = w0 + px:                  entry d exists iff d <= min(ww, D - 1)
    //   right, pixel x = w0 + px - d (px: tile row of the quad's first entry; x >= 0 iff d <= w0 + px):
    //          some entry may exist iff d <= min(w0 + px, D - 1) and px + 3 >= 1, px <= 63; all four exist iff besides
    //          rows px .. px + 3 are rows 1 .. 63 of pixels inside the image (the same in every tile) and d + 3 <= D - 1
    // and the byte offset of a quad within its image row (below 2^31: checked at the entry point) moves by a
    // wave-uniform amount from quad to quad and tile to tile.
    const int q4 = (tid & 15) * 4, sub = tid >> 4;
    const int dlast = ((CVP_ABL & 2) && !cvp_never(D)) ? -1 : D - 1;      // the last disparity that is stored
    int lim_l[4], lim_r[8];
    unsigned whole_r = 0;                       // bit k: rows px .. px + 3 of right quad k are rows 1 .. 63, inside the image
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int px = 1 + sub + 16 * k, ww = w0 + px;
        lim_l[k] = (px < CV_TW && ww < W) ? min(ww, dlast) : -1;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int px = sub + 16 * k - (CV_DT - 1) + q4;
        lim_r[k] = (px + 3 >= 1 && px < CV_TW) ? min(w0 + px, dlast) : -1;
        whole_r |= (px >= 1 && px + 3 < CV_TW && w0 + px + 3 < W) ? 1u << k : 0u;
    }
    const int Dp4 = Dp * 4;
    // (modulo 2^32: a quad outside the image row, never stored, may lie beyond either end)
    const unsigned vo_l = (unsigned)((w0 + 1 + sub) * Dp + q4) * 4u;            // quad 0 of tile 0: pixel w0 + 1 + sub, disparity q4
    const unsigned vo_r = (unsigned)((w0 - (CV_DT - 1) + sub) * Dp + q4) * 4u; //                   pixel w0 - 63 + sub (tile d0: - d0)
    char *const lrow = reinterpret_cast<char *>(lcv + rowbase * Dp), *const rrow = reinterpret_cast<char *>(rcv + rowbase * Dp);
    __syncthreads();
#pragma unroll 1
    for (int d0 = 0; d0 < D && w0 + CV_TW - 1 >= d0; d0 += CV_DT) {   // beyond: every (w, d) has w < d (border fill)
        // the next tile's 64 new columns w0 - d0 - 127 .. w0 - d0 - 64 on their way (4 x 16 bytes per thread; behind the
        // last tile they are fetched for nothing, out of rows the cache holds)
        cv_f4 nx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256, x = w0 - d0 - (2 * CV_DT - 1) + (i >> 4), c4 = i & 15;
            // unconditional (clamped address): a load inside a condition makes the compiler's wait bookkeeping join
            // conservatively, and every later reuse of a register then drains the queue
            nx[q] = *reinterpret_cast<const cv_f4 *>(fr + (rowbase + min(max(x, 0), W - 1)) * CV_C + c4 * 4);
        }
#pragma unroll 1
        for (int kk = 0; kk < (((CVP_ABL & 1) && !cvp_never(D)) ? 0 : 8); ++kk) {
            const int dloc = dq * 16 + 2 * kk;                   // the even disparity of the pair (tile-relative)
            const int r = (w - d0 - dloc) & (RING - 1);          // ring row of right column w - d_even
            const float *b = &sR[r * CV_LD];
            float acc[8], acn[8];                                // this lane's score for d_even; for d_even + 1 (neighbour's row)
            // numpy pairwise_sum, n = 64: r[j] = p[j]; r[j] += p[8i+j]; ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
            // eight channels at a time, the next eight fetched under them
            float4 n0 = *reinterpret_cast<const float4 *>(b), n1 = *reinterpret_cast<const float4 *>(b + 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float bv[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
                if (i < 7) {
                    n0 = *reinterpret_cast<const float4 *>(b + (i + 1) * 8);
                    n1 = *reinterpret_cast<const float4 *>(b + (i + 1) * 8 + 4);
                }
                // the float32 operations of four channels as one block of instructions, independent ones next to each
                // other (the compiler otherwise defers one half of them to the end of the row and keeps - or spills -
                // everything they need until then)
#pragma unroll
                for (int j = 0; j < 8; j += 4) {
                    if (i == 0) {
                        asm volatile("v_mul_f32 %0, %8, %12\n\tv_mul_f32 %1, %9, %13\n\tv_mul_f32 %2, %10, %14\n\tv_mul_f32 %3, %11, %15\n\t"
                                     "v_mul_f32_dpp %4, %12, %8 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %5, %13, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %6, %14, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %7, %15, %11 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                                     : "=&v"(acc[j]), "=&v"(acc[j + 1]), "=&v"(acc[j + 2]), "=&v"(acc[j + 3]),
                                       "=&v"(acn[j]), "=&v"(acn[j + 1]), "=&v"(acn[j + 2]), "=&v"(acn[j + 3])
                                     : "v"(a[j]), "v"(a[j + 1]), "v"(a[j + 2]), "v"(a[j + 3]),
                                       "v"(bv[j]), "v"(bv[j + 1]), "v"(bv[j + 2]), "v"(bv[j + 3]));
                    } else {
                        float t0, t1, t2, t3;
                        asm volatile("v_mul_f32 %8, %12, %16\n\tv_mul_f32 %9, %13, %17\n\tv_mul_f32 %10, %14, %18\n\tv_mul_f32 %11, %15, %19\n\t"
                                     "v_add_f32 %0, %0, %8\n\tv_add_f32 %1, %1, %9\n\tv_add_f32 %2, %2, %10\n\tv_add_f32 %3, %3, %11\n\t"
                                     "v_mul_f32_dpp %8, %16, %12 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %9, %17, %13 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %10, %18, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_mul_f32_dpp %11, %19, %15 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                                     "v_add_f32 %4, %4, %8\n\tv_add_f32 %5, %5, %9\n\tv_add_f32 %6, %6, %10\n\tv_add_f32 %7, %7, %11"
                                     : "+v"(acc[j]), "+v"(acc[j + 1]), "+v"(acc[j + 2]), "+v"(acc[j + 3]),
                                       "+v"(acn[j]), "+v"(acn[j + 1]), "+v"(acn[j + 2]), "+v"(acn[j + 3]),
                                       "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                                     : "v"(a[i * 8 + j]), "v"(a[i * 8 + j + 1]), "v"(a[i * 8 + j + 2]), "v"(a[i * 8 + j + 3]),
                                       "v"(bv[j]), "v"(bv[j + 1]), "v"(bv[j + 2]), "v"(bv[j + 3]));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
            float sn = ((acn[0] + acn[1]) + (acn[2] + acn[3])) + ((acn[4] + acn[5]) + (acn[6] + acn[7]));
            s = 0.f + s;  // np.sum adds the pairwise result to the identity
            sn = 0.f + sn;
            s = -1.f * s;
            sn = -1.f * sn;
            const int d = d0 + dloc;
            if (wl >= 1 && w < W) {
                if (d < D && w >= d) sT[wl * TP + dloc] = s;
                if (d + 1 < D && w >= d + 1) sT[wl * TP + dloc + 1] = sn;
            }
        }
        __syncthreads();                             // products done: the score tile is complete, the oldest ring rows are free
        // (without a next tile the rows written here are never read: the write stays unconditional like its loads)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256, x = w0 - d0 - (2 * CV_DT - 1) + (i >> 4), c4 = i & 15;
            *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + c4 * 4]) = nx[q];
        }
        const int d = d0 + q4;                       // the first disparity of this thread's quads
        unsigned rag = 0;                            // this thread's ragged quads: bits 0 .. 3 left, 4 .. 11 right
        {   // left volume: pixel w0 + px (px >= 1), disparities d0 .. d0 + nd - 1 (those with d <= w)
            cv_f4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                v[k] = *reinterpret_cast<const cv_f4 *>(&sT[min(1 + sub + 16 * k, CV_TW - 1) * TP + q4]);
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(v[k]));   // the reads stay ahead of the first store
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool full = d + 3 <= lim_l[k];
                if (__builtin_expect(full, 1)) cvp_store16(lrow + (vo_l + (unsigned)(d0 * 4 + k * 16 * Dp4)), v[k]);
                rag |= (d <= lim_l[k] && !full) ? 1u << k : 0u;
            }
        }
        {   // right volume: pixel x = w - d; its entries of this tile are (w = x + d, d), d0 <= d < d0 + nd: the score
            // tile's anti-diagonals (four LDS reads per 16-byte store), in two groups of four quads: eight would not
            // fit into the registers beside the left features
#pragma unroll
            for (int k0 = 0; k0 < 8; k0 += 4) {
                cv_f4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pc = min(max(sub + 16 * (k0 + k) - (CV_DT - 1) + q4, 0), CV_TW - 4);
                    v[k].x = sT[pc * TP + q4];
                    v[k].y = sT[(pc + 1) * TP + q4 + 1];
                    v[k].z = sT[(pc + 2) * TP + q4 + 2];
                    v[k].w = sT[(pc + 3) * TP + q4 + 3];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(v[k]));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool some = d <= lim_r[k0 + k];
                    const bool full = some && ((whole_r >> (k0 + k)) & 1) && d + 3 <= dlast;
                    if (__builtin_expect(full, 1))
                        cvp_store16(rrow + (vo_r + (unsigned)(d0 * 4 + ((k0 + k) * 16 - d0) * Dp4)), v[k]);
                    rag |= (some && !full) ? 16u << (k0 + k) : 0u;
                }
            }
        }
        // the ragged quads, one per turn (few threads have any, and hardly one has more than two)
        for (unsigned m = rag & 15u; m; m &= m - 1) {
            const int k = __builtin_ctz(m), px = 1 + sub + 16 * k, lim = min(w0 + px, dlast);
            float *dst = reinterpret_cast<float *>(lrow + (vo_l + (unsigned)(d0 * 4 + k * 16 * Dp4)));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (d + j <= lim) dst[j] = sT[px * TP + q4 + j];
        }
        for (unsigned m = rag >> 4; m; m &= m - 1) {
            const int k = __builtin_ctz(m), px = sub + 16 * k - (CV_DT - 1) + q4;
            float *dst = reinterpret_cast<float *>(rrow + (vo_r + (unsigned)(d0 * 4 + (k * 16 - d0) * Dp4)));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (d + j <= dlast && px + j >= 1 && px + j < CV_TW && w0 + px + j < W) dst[j] = sT[(px + j) * TP + q4 + j];
        }
        __syncthreads();                             // the score tile has been read, the ring holds the next tile's rows
    }
}

// ---- vertical search (include/mccnn.h: mccnn_cost_volume_vertical_hwd) ------------------------------------------------
// S_L(d,h,w) = max_k P(k; d,h,w) pairs left pixel (h,w) with right pixels (h+k, w-d); S_R(d,h,w) pairs right pixel (h,w)
// with left pixels (h-k, w+d).  Seen from its own pixel, either view is the same job: the pixel's features stay in
// registers, the OTHER view's rows h +- k are searched, and only the pixel's OWN volume is written - for k != 0 an
// entry of the other volume takes its maximum over other products, so nothing but k = 0 is shared and the scatter
// along the score tile's anti-diagonals, half of cost_volume_exact_pairs_kernel's store phase, has nothing to carry.
// Hence ONE kernel launched for both views (blockIdx.z): the right view is the left view's code on the horizontally
// mirrored pair with the roles of the images swapped - "search column" c is image column c on the left and W - 1 - c on
// the right, where the match of search column c at disparity d lies at search column c - d in both - and with the
// candidate rows walked the other way (row h - k for ascending k).  Products commute, so the 64 rounded products and
// their summation order per score are those of the pairs kernel: the same ghost lane, the same DPP operand, the same
// ring indexed by (search column & 127).
// What the vertical search costs in LDS: the ring would have to exist once per candidate row for a tile's 63 reusable
// columns to survive until the next tile, 34 KiB each - beside the 17 KiB left tile that is one workgroup per CU at
// r = 2.  So the ring is re-staged for every (tile, candidate): all 128 rows (8 x 16 bytes per thread, out of rows the
// L2 holds: a workgroup reads each of its 2r + 1 rows once per tile) instead of the 64 new ones, fetched into
// registers under the products of the candidate before and written behind them.  The running maximum lives in the
// score tile: entry (wl, d) is read, compared and written by the one thread that computes it, so the candidates need
// no synchronisation beyond the ring's, and every voxel is stored once, behind the last candidate, negated there.
// Both launches together do 2 (2r + 1) = 4r + 2 product sets; the k = 0 set is computed once per view.
__device__ __forceinline__ void cvv_pair_scores(const float (&a)[CV_C], const float *b, float &s_out, float &sn_out)
{
    float acc[8], acn[8];                                // this lane's score for d_even; for d_even + 1 (neighbour's row)
    // numpy pairwise_sum, n = 64, as in cost_volume_exact_pairs_kernel: the same instruction blocks
    float4 n0 = *reinterpret_cast<const float4 *>(b), n1 = *reinterpret_cast<const float4 *>(b + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float bv[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
        if (i < 7) {
            n0 = *reinterpret_cast<const float4 *>(b + (i + 1) * 8);
            n1 = *reinterpret_cast<const float4 *>(b + (i + 1) * 8 + 4);
        }
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
            if (i == 0) {
                asm volatile("v_mul_f32 %0, %8, %12\n\tv_mul_f32 %1, %9, %13\n\tv_mul_f32 %2, %10, %14\n\tv_mul_f32 %3, %11, %15\n\t"
                             "v_mul_f32_dpp %4, %12, %8 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %5, %13, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %6, %14, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %7, %15, %11 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                             : "=&v"(acc[j]), "=&v"(acc[j + 1]), "=&v"(acc[j + 2]), "=&v"(acc[j + 3]),
                               "=&v"(acn[j]), "=&v"(acn[j + 1]), "=&v"(acn[j + 2]), "=&v"(acn[j + 3])
                             : "v"(a[j]), "v"(a[j + 1]), "v"(a[j + 2]), "v"(a[j + 3]),
                               "v"(bv[j]), "v"(bv[j + 1]), "v"(bv[j + 2]), "v"(bv[j + 3]));
            } else {
                float t0, t1, t2, t3;
                asm volatile("v_mul_f32 %8, %12, %16\n\tv_mul_f32 %9, %13, %17\n\tv_mul_f32 %10, %14, %18\n\tv_mul_f32 %11, %15, %19\n\t"
                             "v_add_f32 %0, %0, %8\n\tv_add_f32 %1, %1, %9\n\tv_add_f32 %2, %2, %10\n\tv_add_f32 %3, %3, %11\n\t"
                             "v_mul_f32_dpp %8, %16, %12 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %9, %17, %13 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %10, %18, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_mul_f32_dpp %11, %19, %15 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_add_f32 %4, %4, %8\n\tv_add_f32 %5, %5, %9\n\tv_add_f32 %6, %6, %10\n\tv_add_f32 %7, %7, %11"
                             : "+v"(acc[j]), "+v"(acc[j + 1]), "+v"(acc[j + 2]), "+v"(acc[j + 3]),
                               "+v"(acn[j]), "+v"(acn[j + 1]), "+v"(acn[j + 2]), "+v"(acn[j + 3]),
                               "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                             : "v"(a[i * 8 + j]), "v"(a[i * 8 + j + 1]), "v"(a[i * 8 + j + 2]), "v"(a[i * 8 + j + 3]),
                               "v"(bv[j]), "v"(bv[j + 1]), "v"(bv[j + 2]), "v"(bv[j + 3]));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    const float sn = ((acn[0] + acn[1]) + (acn[2] + acn[3])) + ((acn[4] + acn[5]) + (acn[6] + acn[7]));
    s_out = 0.f + s;  // np.sum adds the pairwise result to the identity
    sn_out = 0.f + sn;
}

// the definition's maximum: a candidate replaces the best so far when it is larger or NaN (NaN then stays: nothing is
// larger than it, and a later NaN is NaN again); among equal values the first one seen is kept
__device__ __forceinline__ void cvv_take(float *best, float s, bool first)
{
    const float b = first ? s : *best;
    *best = (s > b || s != s) ? s : b;
}

// OFFSET (include/mccnn.h: mccnn_cost_volume_offset_hwd): the candidates lie around k0 = *row_offset clamped to +-8
// instead of around 0 - only klo / khi differ; a row none of whose candidates lies inside the image takes the one
// candidate nearest to k0 that does.  The search itself (OFFSET = false) is the kernel as it was.
//
// FIELD (include/mccnn.h: mccnn_cost_volume_field_hwd): the offset is a word of a gh x gw grid, F, chosen per ENTRY - by
// the pixel's own column in the left view, by its partner's column w + d in the right view - so the entries of one score
// tile may lie around different offsets.  The candidates of a disparity tile are then a SET (cvf_tile: the union, over
// the at most three 64-column blocks the tile's entries choose from, of the candidates around each block's offset),
// walked in ascending order like klo .. khi, and an entry's running maximum takes candidate k only where k is one of the
// entry's own - its range is contiguous and part of the set, so it meets them in the definition's order.  A tile whose
// blocks agree (nearly all of them) takes the comparisons of OFFSET: one range for every entry.  `vrange` carries the
// grid: range | gh << 8 | gw << 16; `row_offset` is the field.  Every candidate of the set lies in [kmin, kmax] by
// construction, whatever the field's words hold, so no row index leaves the image.
struct cvf_tile_t {
    unsigned mask;          // bit k + CVF_BIAS: candidate k is some entry's
    int blo;                // the first block of image columns the tile's entries choose from
    int f0, f1, f2;         // the clamped field words of blocks blo, blo + 1, blo + 2
    int lo, hi;             // block blo's candidates: every entry's where `same`
    int same;               // the blocks in use agree (an int: the struct has no padding to copy)
};
constexpr int CVF_BIAS = MCCNN_VERTICAL_OFFSET_MAX + MCCNN_VERTICAL_RANGE_MAX;

// the candidates around offset f: k = f - r .. f + r inside [kmin, kmax], else the one nearest to f
__device__ __forceinline__ void cvf_range(int f, int r, int kmin, int kmax, int &lo, int &hi)
{
    lo = max(f - r, kmin);
    hi = min(f + r, kmax);
    if (lo > hi) lo = hi = min(max(f, kmin), kmax);
}

template <bool OFFSET, bool FIELD = false>
__global__ __launch_bounds__(256, 3) void cost_volume_vertical_kernel(const float *__restrict__ fl,
                                                                      const float *__restrict__ fr, int H, int W, int D,
                                                                      int vrange, float *__restrict__ lcv,
                                                                      float *__restrict__ rcv, int Dp,
                                                                      const int *__restrict__ row_offset)
{
    constexpr int RING = 128;
    __shared__ __attribute__((aligned(16))) float sR[RING * CV_LD];
    __shared__ __attribute__((aligned(16))) float sL[CV_TW * CV_LD];
    const bool right = blockIdx.z != 0;                 // the view whose volume this workgroup writes
    const float *const fa = right ? fr : fl;            // its own features (registers) ...
    const float *const fb = right ? fl : fr;            // ... and the other view's (ring)
    const int mir = right ? W - 1 : 0, sgn = right ? -1 : 1;   // image column of search column c: mir + sgn * c
    const int w0 = (int)blockIdx.x * CVP_TW - 1, h = blockIdx.y;   // lane 0: search column w0 (ghost)
    const int tid = threadIdx.x;
    const int gh = FIELD ? (vrange >> 8) & 0xff : 1, gw = FIELD ? (vrange >> 16) & 0xff : 1;
    if (FIELD) vrange &= 0xff;
    // the candidates k = klo .. khi, ascending: the other view's row h + sgn * k lies inside the image (k = 0 always does)
    int klo = right ? max(-vrange, h - (H - 1)) : max(-vrange, -h);
    int khi = right ? min(vrange, h) : min(vrange, H - 1 - h);
    // FIELD: what disparity tile d0 of this workgroup meets.  Its entries (ww, d) - search column ww = w0 + 1 .. w0 + 63
    // inside the image, d = d0 .. min(d0 + 63, D - 1), d <= ww - choose by image column ww (left view) or by the image
    // column of search column ww - d (right view): an interval of at most 126 columns, three blocks.
    const int nb = (W + 63) >> 6;
    const int kmin = right ? h - (H - 1) : -h, kmax = right ? h : H - 1 - h;     // the k whose row is an image row
    const int *const frow = FIELD ? row_offset + (h * gh / H) * gw : nullptr;     // the row band of h: gw words
    auto cvf_tile = [&](int d0) {
        cvf_tile_t t;
        const int whi = min(w0 + CV_TW - 1, W - 1);
        int clo = max(w0 + 1, d0), chi = whi;                                     // left view: the columns with an entry
        if (right) {
            clo = max(w0 + 1 - min(d0 + CV_DT - 1, D - 1), 0);
            chi = whi - d0;
        }
        const int xlo = right ? W - 1 - chi : clo, xhi = right ? W - 1 - clo : chi;
        t.blo = min(max(xlo, 0), W - 1) >> 6;
        const int nblk = clo > chi ? 0 : (min(max(xhi, 0), W - 1) >> 6) - t.blo + 1;
        t.mask = 0u;
        t.same = 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int word = frow[min(t.blo + j, nb - 1) * gw / nb];
            const int f = min(max(word, -MCCNN_VERTICAL_OFFSET_MAX), MCCNN_VERTICAL_OFFSET_MAX);   // any stored value is safe
            int lo, hi;
            cvf_range(f, vrange, kmin, kmax, lo, hi);
            if (j == 0) {
                t.f0 = f;
                t.lo = lo;
                t.hi = hi;
            }
            if (j == 1) t.f1 = f;
            if (j == 2) t.f2 = f;
            if (j < nblk) {
                t.mask |= (2u << (hi + CVF_BIAS)) - (1u << (lo + CVF_BIAS));
                t.same &= f == t.f0;
            }
        }
        if (t.mask == 0u) t.mask = 1u << CVF_BIAS;      // no entry at all: k = 0 runs, nothing is kept or stored
        return t;
    };
    if (OFFSET) {
        const int k0 = min(max(*row_offset, -MCCNN_VERTICAL_OFFSET_MAX), MCCNN_VERTICAL_OFFSET_MAX);   // any stored value is safe
        const int kmin = right ? h - (H - 1) : -h, kmax = right ? h : H - 1 - h;     // the k whose row is an image row
        klo = max(k0 - vrange, kmin);
        khi = min(k0 + vrange, kmax);
        if (klo > khi) klo = khi = min(max(k0, kmin), kmax);
    }
    if (FIELD) klo = __builtin_ctz(cvf_tile(0).mask) - CVF_BIAS;      // the first candidate of the first tile
    // the 16 bytes at channels 4 c4 .. of search column c (clamped: kept as it comes, never part of a stored score)
    auto at = [&](const float *f, int row, int c, int c4) {
        return reinterpret_cast<const cv_f4 *>(f + ((size_t)row * W + (mir + sgn * min(max(c, 0), W - 1))) * CV_C + c4 * 4);
    };
    {
        cv_f4 pl[4], pr[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256;
            pl[q] = *at(fa, h, w0 + (i >> 4), i & 15);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {     // the first tile's search columns w0 - 63 .. w0 + 64 of the first candidate's row
            const int i = tid + q * 256;
            pr[q] = *at(fb, h + sgn * klo, w0 - (CV_DT - 1) + (i >> 4), i & 15);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256;
            *reinterpret_cast<cv_f4 *>(&sL[(i >> 4) * CV_LD + (i & 15) * 4]) = pl[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + q * 256, x = w0 - (CV_DT - 1) + (i >> 4);
            *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = pr[q];
        }
    }
    __syncthreads();

    const int wl = tid & 63, dq = tid >> 6;  // dq is wave-uniform: each wave owns 16 disparities = 8 pairs of a tile
    const int w = w0 + wl;
    float a[CV_C];
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
        const float4 v = *reinterpret_cast<const float4 *>(&sL[wl * CV_LD + c4 * 4]);
        a[c4 * 4 + 0] = v.x; a[c4 * 4 + 1] = v.y; a[c4 * 4 + 2] = v.z; a[c4 * 4 + 3] = v.w;
    }
    constexpr int TP = CV_LD;
    float *const sT = sL;               // every thread holds its own features in registers from here on
    // The store phase is the pairs kernel's for its left volume: 16 lanes x four disparities = one pixel's 64
    // disparities of a tile, a thread owns 4 quads per tile; FULL quads leave as one 16-byte store, a quad that
    // straddles w = d or the last disparity goes out float by float.  Entry d of search column ww exists iff
    // d <= min(ww, D - 1), in either view.
    const int q4 = (tid & 15) * 4, sub = tid >> 4;
    const int dlast = D - 1;
    const int Dp4 = Dp * 4;
    // byte offset of quad 0 of tile 0 within the image row (below 2^31: checked at the entry point; modulo 2^32 for a
    // quad outside the row, which is never stored); the next quad is 16 search columns on: 16 pixels up or down
    const unsigned vo = (unsigned)((mir + sgn * (w0 + 1 + sub)) * Dp + q4) * 4u;
    char *const vrow = reinterpret_cast<char *>((right ? rcv : lcv) + (size_t)h * W * Dp);
    __syncthreads();
    if constexpr (FIELD) {
        // the search's loops over a SET of candidates per tile; an entry takes candidate k only where k is its own
        cvf_tile_t cur = cvf_tile(0);                   // (klo: its first candidate - the prologue staged that row)
#pragma unroll 1
        for (int d0 = 0; d0 < D && w0 + CV_TW - 1 >= d0; d0 += CV_DT) {
            const bool more = d0 + CV_DT < D && w0 + CV_TW - 1 >= d0 + CV_DT;
            const cvf_tile_t nxt = more ? cvf_tile(d0 + CV_DT) : cur;     // (behind the last tile: fetched for nothing)
#pragma unroll 1
            for (unsigned m = cur.mask; m;) {           // ascending
                const int k = __builtin_ctz(m) - CVF_BIAS;
                m &= m - 1;
                const bool last = m == 0u;
                const int nd0 = last ? d0 + CV_DT : d0, nrow = h + sgn * (__builtin_ctz(last ? nxt.mask : m) - CVF_BIAS);
                cv_f4 nx[4], ny[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = tid + q * 256;
                    nx[q] = *at(fb, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
                }
#pragma unroll 1
                for (int kk = 0; kk < 8; ++kk) {
                    const int dloc = dq * 16 + 2 * kk;                   // the even disparity of the pair (tile-relative)
                    const int r = (w - d0 - dloc) & (RING - 1);          // ring row of search column w - d_even
                    float s, sn;
                    cvv_pair_scores(a, &sR[r * CV_LD], s, sn);
                    const int d = d0 + dloc;
                    int lo = cur.lo, hi = cur.hi, lon = lo, hin = hi;       // this entry's candidates, and d + 1's
                    if (!cur.same) {                     // (uniform) the entries choose by their columns
                        const int x = right ? W - 1 - (w - d) : w;
                        const int b = min(max((x >> 6) - cur.blo, 0), 2);
                        const int bn = right ? min(max(((x + 1) >> 6) - cur.blo, 0), 2) : b;    // its partner: one column on
                        cvf_range(b == 0 ? cur.f0 : (b == 1 ? cur.f1 : cur.f2), vrange, kmin, kmax, lo, hi);
                        cvf_range(bn == 0 ? cur.f0 : (bn == 1 ? cur.f1 : cur.f2), vrange, kmin, kmax, lon, hin);
                    }
                    if (wl >= 1 && w < W) {
                        if (d < D && w >= d && k >= lo && k <= hi) cvv_take(&sT[wl * TP + dloc], s, k == lo);
                        if (d + 1 < D && w >= d + 1 && k >= lon && k <= hin) cvv_take(&sT[wl * TP + dloc + 1], sn, k == lon);
                    }
                }
                __syncthreads();                         // this candidate's products are done: the ring is free
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = tid + (q + 4) * 256;
                    ny[q] = *at(fb, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = tid + q * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                    *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = nx[q];
                }
                if (last) {                            // the score tile holds the maxima: negate (pf:111-112) and store
                    const int d = d0 + q4;               // the first disparity of this thread's quads
                    unsigned rag = 0;
                    cv_f4 v[4];
                    int lim[4];                          // (worked out per tile: four registers less across the products)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int px = 1 + sub + 16 * j, ww = w0 + px;
                        lim[j] = (px < CV_TW && ww < W) ? min(ww, dlast) : -1;
                        v[j] = *reinterpret_cast<const cv_f4 *>(&sT[min(px, CV_TW - 1) * TP + q4]);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool full = d + 3 <= lim[j];
                        if (__builtin_expect(full, 1))
                            cvp_store16(vrow + (vo + (unsigned)(d0 * 4 + sgn * j * 16 * Dp4)), -1.f * v[j]);
                        rag |= (d <= lim[j] && !full) ? 1u << j : 0u;
                    }
                    for (unsigned m = rag; m; m &= m - 1) {
                        const int j = __builtin_ctz(m), px = 1 + sub + 16 * j;
                        float *dst = reinterpret_cast<float *>(vrow + (vo + (unsigned)(d0 * 4 + sgn * j * 16 * Dp4)));
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (d + e <= lim[j]) dst[e] = -1.f * sT[px * TP + q4 + e];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = tid + (q + 4) * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                    *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = ny[q];
                }
                __syncthreads();                    // the ring holds the next candidate's rows, the score tile has been read
            }
            cur = nxt;
        }
        return;
    }
#pragma unroll 1
    for (int d0 = 0; d0 < D && w0 + CV_TW - 1 >= d0; d0 += CV_DT) {   // beyond: every (w, d) has w < d (border fill)
#pragma unroll 1
        for (int k = klo; k <= khi; ++k) {
            const bool first = k == klo, last = k == khi;
            // the rows of the next (tile, candidate) on their way; behind the last one they are fetched for nothing
            const int nd0 = last ? d0 + CV_DT : d0, nrow = h + sgn * (last ? klo : k + 1);
            // (their first half under the products, like the pairs kernel's four; all eight beside the own features do
            // not fit into the registers of three workgroups per CU - 40 bytes of scratch - so the second half is
            // fetched behind the products and lands under the tile's stores)
            cv_f4 nx[4], ny[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + q * 256;
                nx[q] = *at(fb, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
            }
#pragma unroll 1
            for (int kk = 0; kk < 8; ++kk) {
                const int dloc = dq * 16 + 2 * kk;                   // the even disparity of the pair (tile-relative)
                const int r = (w - d0 - dloc) & (RING - 1);          // ring row of search column w - d_even
                float s, sn;
                cvv_pair_scores(a, &sR[r * CV_LD], s, sn);
                const int d = d0 + dloc;
                if (wl >= 1 && w < W) {
                    if (d < D && w >= d) cvv_take(&sT[wl * TP + dloc], s, first);
                    if (d + 1 < D && w >= d + 1) cvv_take(&sT[wl * TP + dloc + 1], sn, first);
                }
            }
            __syncthreads();                         // this candidate's products are done: the ring is free
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + (q + 4) * 256;
                ny[q] = *at(fb, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + q * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = nx[q];
            }
            if (last) {                            // the score tile holds the maxima: negate (pf:111-112) and store
                const int d = d0 + q4;               // the first disparity of this thread's quads
                unsigned rag = 0;
                cv_f4 v[4];
                int lim[4];                          // (worked out per tile: four registers less across the products)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = 1 + sub + 16 * j, ww = w0 + px;
                    lim[j] = (px < CV_TW && ww < W) ? min(ww, dlast) : -1;
                    v[j] = *reinterpret_cast<const cv_f4 *>(&sT[min(px, CV_TW - 1) * TP + q4]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool full = d + 3 <= lim[j];
                    if (__builtin_expect(full, 1))
                        cvp_store16(vrow + (vo + (unsigned)(d0 * 4 + sgn * j * 16 * Dp4)), -1.f * v[j]);
                    rag |= (d <= lim[j] && !full) ? 1u << j : 0u;
                }
                for (unsigned m = rag; m; m &= m - 1) {
                    const int j = __builtin_ctz(m), px = 1 + sub + 16 * j;
                    float *dst = reinterpret_cast<float *>(vrow + (vo + (unsigned)(d0 * 4 + sgn * j * 16 * Dp4)));
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (d + e <= lim[j]) dst[e] = -1.f * sT[px * TP + q4 + e];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + (q + 4) * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = ny[q];
            }
            __syncthreads();                        // the ring holds the next candidate's rows, the score tile has been read
        }
    }
}

// ---- the row offset of a pair, measured (include/mccnn.h: mccnn_vertical_profile, mccnn_vertical_offset_select) --------
// One workgroup per (63-pixel tile, profiled row) of the LEFT view: the tile, ring and product block of the search
// above, and no volume.  Candidates outermost, in the order of the vote (0, -1, +1, ...): for one candidate a thread
// keeps the maximum over its wave's 16 disparities of every disparity tile in a register; the four waves' maxima of a
// pixel meet in the score tile's LDS (free once the own features are in registers) and wave 0 keeps (best value, best k,
// NaN seen) per pixel.  The maximum's rule makes NaN sticky, so b(k) is NaN iff one of its scores is; which of several
// equal scores is kept is invisible to the comparisons that follow.  The ring is re-staged per (candidate, disparity
// tile) exactly as above.  The votes of a tile (it touches at most two 64-pixel blocks) are counted in LDS and leave as
// at most 2 (2R + 1) integer atomics per workgroup: the result does not depend on any order.
__device__ __forceinline__ int cvp_candidate(int c) { return c == 0 ? 0 : ((c & 1) ? -((c + 1) >> 1) : (c >> 1)); }

__global__ __launch_bounds__(256, 3) void vertical_profile_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                                  int H, int W, int D, int R, int row_step,
                                                                  unsigned *__restrict__ votes, int n_blocks)
{
    constexpr int RING = 128, NK = 2 * MCCNN_VERTICAL_OFFSET_MAX + 1;
    __shared__ __attribute__((aligned(16))) float sR[RING * CV_LD];
    __shared__ __attribute__((aligned(16))) float sL[CV_TW * CV_LD];
    __shared__ unsigned sH[2 * NK];
    const int w0 = (int)blockIdx.x * CVP_TW - 1, h = row_step / 2 + (int)blockIdx.y * row_step;   // h < H: the grid's rows
    const int tid = threadIdx.x;
    const int nk = 2 * R + 1;
    auto at = [&](const float *f, int row, int c, int c4) {
        return reinterpret_cast<const cv_f4 *>(f + ((size_t)row * W + min(max(c, 0), W - 1)) * CV_C + c4 * 4);
    };
    // the candidate behind candidate c whose row lies inside the image; 2R + 1: none
    auto next_candidate = [&](int c) {
        for (++c; c < nk; ++c) {
            const int row = h + cvp_candidate(c);
            if (row >= 0 && row < H) break;
        }
        return c;
    };
    if (tid < 2 * NK) sH[tid] = 0u;
    {
        cv_f4 pl[4], pr[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256;
            pl[q] = *at(fl, h, w0 + (i >> 4), i & 15);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {     // the first tile's columns w0 - 63 .. w0 + 64 of the first candidate's row (k = 0)
            const int i = tid + q * 256;
            pr[q] = *at(fr, h, w0 - (CV_DT - 1) + (i >> 4), i & 15);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * 256;
            *reinterpret_cast<cv_f4 *>(&sL[(i >> 4) * CV_LD + (i & 15) * 4]) = pl[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + q * 256, x = w0 - (CV_DT - 1) + (i >> 4);
            *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = pr[q];
        }
    }
    __syncthreads();

    const int wl = tid & 63, dq = tid >> 6;  // dq is wave-uniform: each wave owns 16 disparities = 8 pairs of a tile
    const int w = w0 + wl;
    const bool pixel = wl >= 1 && w < W;     // lane 0 is the ghost
    float a[CV_C];
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
        const float4 v = *reinterpret_cast<const float4 *>(&sL[wl * CV_LD + c4 * 4]);
        a[c4 * 4 + 0] = v.x; a[c4 * 4 + 1] = v.y; a[c4 * 4 + 2] = v.z; a[c4 * 4 + 3] = v.w;
    }
    float *const sM = sL;               // [4][64]: the four waves' maxima of the current candidate
    __syncthreads();
    float best = 0.f;
    int bestk = 0;
    bool nan_seen = false;
#pragma unroll 1
    for (int c = 0; c < nk;) {
        const int k = cvp_candidate(c), nc = next_candidate(c);
        float m = -__builtin_inff();         // below every score; d = 0 exists for every pixel
#pragma unroll 1
        for (int d0 = 0; d0 < D && w0 + CV_TW - 1 >= d0; d0 += CV_DT) {
            const bool lastd = !(d0 + CV_DT < D && w0 + CV_TW - 1 >= d0 + CV_DT);
            // the rows of the next (candidate, tile) on their way; behind the last one they are fetched for nothing
            const int nd0 = lastd ? 0 : d0 + CV_DT, nrow = h + (lastd ? (nc < nk ? cvp_candidate(nc) : 0) : k);
            cv_f4 nx[4], ny[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + q * 256;
                nx[q] = *at(fr, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
            }
#pragma unroll 1
            for (int kk = 0; kk < 8; ++kk) {
                const int dloc = dq * 16 + 2 * kk;
                const int r = (w - d0 - dloc) & (RING - 1);
                float s, sn;
                cvv_pair_scores(a, &sR[r * CV_LD], s, sn);
                const int d = d0 + dloc;
                if (pixel && d < D && w >= d) m = (s > m || s != s) ? s : m;
                if (pixel && d + 1 < D && w >= d + 1) m = (sn > m || sn != sn) ? sn : m;
            }
            __syncthreads();                         // this tile's products are done: the ring is free
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + (q + 4) * 256;
                ny[q] = *at(fr, nrow, w0 - nd0 - (CV_DT - 1) + (i >> 4), i & 15);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + q * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = nx[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = tid + (q + 4) * 256, x = w0 - nd0 - (CV_DT - 1) + (i >> 4);
                *reinterpret_cast<cv_f4 *>(&sR[(x & (RING - 1)) * CV_LD + (i & 15) * 4]) = ny[q];
            }
            __syncthreads();                        // the ring holds the next tile's rows
        }
        sM[dq * 64 + wl] = m;       // (last read two barriers ago: every candidate runs at least the tile d0 = 0)
        __syncthreads();
        if (dq == 0) {
            float b = sM[wl];       // waves in ascending order: d ascending
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const float s = sM[q * 64 + wl];
                b = (s > b || s != s) ? s : b;
            }
            nan_seen = nan_seen || b != b;
            if (c == 0 || b > best) {
                best = b;
                bestk = k;
            }
        }
        c = nc;
    }
    if (dq == 0 && pixel && !nan_seen) atomicAdd(&sH[((w >> 6) - ((w0 + 1) >> 6)) * NK + bestk + R], 1u);
    __syncthreads();
    if (tid < 2 * NK) {
        const int blk = ((w0 + 1) >> 6) + tid / NK, kk = tid % NK;
        const unsigned n = sH[tid];
        if (n != 0u && blk < n_blocks && kk < nk) atomicAdd(&votes[((size_t)blockIdx.y * n_blocks + blk) * nk + kk], n);
    }
}

// totals[k + R] = the votes for k over all rows and blocks; *offset = the k of the largest total (candidates 0, -1, +1,
// ..., replaced only by a strictly greater total: no votes at all give 0).  One workgroup; integer sums only.
__global__ __launch_bounds__(256) void vertical_offset_select_kernel(const unsigned *__restrict__ votes, int n_cells, int R,
                                                                     int *__restrict__ offset,
                                                                     unsigned long long *__restrict__ totals)
{
    constexpr int NK = 2 * MCCNN_VERTICAL_OFFSET_MAX + 1;
    __shared__ unsigned long long sT[NK];
    const int nk = 2 * R + 1;
    if (threadIdx.x < NK) sT[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long acc[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) acc[j] = 0ull;
    for (int cell = threadIdx.x; cell < n_cells; cell += 256)
#pragma unroll
        for (int j = 0; j < NK; ++j)
            if (j < nk) acc[j] += votes[(size_t)cell * nk + j];
#pragma unroll
    for (int j = 0; j < NK; ++j)
        if (j < nk && acc[j] != 0ull) atomicAdd(&sT[j], acc[j]);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = sT[R];
        int k0 = 0;
        for (int c = 1; c < nk; ++c) {
            const int k = cvp_candidate(c);
            if (sT[k + R] > best) {
                best = sT[k + R];
                k0 = k;
            }
        }
        *offset = k0;
    }
    if ((int)threadIdx.x < nk) totals[threadIdx.x] = sT[threadIdx.x];
}

// The same selection per cell of a gh x gw grid (include/mccnn.h: mccnn_vertical_field_select): profiled row i belongs
// to row band h_i gh / H, block blk to column band blk gw / n_blocks.  One workgroup; the cells' totals are summed in LDS
// by integer atomics (at most 64 cells, 17 candidates each), so the result depends on no order; the whole image's are the
// cells' sums.  A cell without a vote takes the whole image's winner, which is mccnn_vertical_offset_select's.
__device__ __forceinline__ int cvp_winner(const unsigned long long *t, int R)
{
    unsigned long long best = t[R];
    int k0 = 0;
    for (int c = 1; c < 2 * R + 1; ++c) {
        const int k = cvp_candidate(c);
        if (t[k + R] > best) {
            best = t[k + R];
            k0 = k;
        }
    }
    return k0;
}

__global__ __launch_bounds__(256) void vertical_field_select_kernel(const unsigned *__restrict__ votes, int n_rows,
                                                                    int n_blocks, int H, int row_step, int R, int gh, int gw,
                                                                    int *__restrict__ field,
                                                                    unsigned long long *__restrict__ totals,
                                                                    int *__restrict__ offset,
                                                                    unsigned long long *__restrict__ global_totals)
{
    constexpr int NK = 2 * MCCNN_VERTICAL_OFFSET_MAX + 1, CELLS = MCCNN_VERTICAL_FIELD_MAX * MCCNN_VERTICAL_FIELD_MAX;
    __shared__ unsigned long long sT[(CELLS + 1) * NK];       // [cell][k + R]; the last one: the whole image
    __shared__ int sG;
    const int nk = 2 * R + 1, cells = gh * gw, tid = threadIdx.x;
    for (int i = tid; i < (cells + 1) * NK; i += 256) sT[i] = 0ull;
    __syncthreads();
    for (int v = tid; v < n_rows * n_blocks; v += 256) {
        const int i = v / n_blocks, blk = v - i * n_blocks;
        const long long hi = (long long)(row_step / 2) + (long long)i * row_step;                  // h_i < H
        const int a = min(H < (1 << 27) ? (int)((unsigned)hi * (unsigned)gh / (unsigned)H) : (int)(hi * gh / H), gh - 1);
        const int cell = a * gw + blk * gw / n_blocks;
        unsigned n[NK];                          // the loads first, all in flight; then the cell's atomics
#pragma unroll
        for (int j = 0; j < NK; ++j) n[j] = j < nk ? votes[(size_t)v * nk + j] : 0u;
#pragma unroll
        for (int j = 0; j < NK; ++j)
            if (n[j] != 0u) atomicAdd(&sT[cell * NK + j], (unsigned long long)n[j]);
    }
    __syncthreads();
    if (tid < nk) {                              // the whole image: the sum of the cells, beside them (no contended word)
        unsigned long long all = 0ull;
        for (int c = 0; c < cells; ++c) all += sT[c * NK + tid];
        sT[cells * NK + tid] = all;
    }
    __syncthreads();
    if (tid == 0) sG = cvp_winner(&sT[cells * NK], R);
    __syncthreads();
    if (tid < cells) {
        unsigned long long any = 0ull;
        for (int j = 0; j < nk; ++j) any |= sT[tid * NK + j];
        field[tid] = any != 0ull ? cvp_winner(&sT[tid * NK], R) : sG;
    }
    for (int i = tid; i < cells * nk; i += 256) totals[i] = sT[(i / nk) * NK + i % nk];
    if (tid < nk) global_totals[tid] = sT[cells * NK + tid];
    if (tid == 0) *offset = sG;
}

// ---- MFMA variant ---------------------------------------------------------------------------------------------
// One wave computes a 32(w) x 32(w') block of S = <fl[w], fr[w']>; a workgroup of 4 waves covers 64 w x 64 w' and
// keeps only the band 0 <= w-w' < D.  A/B operands: lane l holds pixel l&31, channels 8 (l>>5) .. +7 of a 16-channel
// K step; C/D: col = lane&31 (w'), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (w).
//
// What bounds this kernel is neither the matrix cores nor the store pattern but how many workgroups a CU can hold:
// a workgroup is a chain of latencies (operand fetch, LDS staging, products, the transposition through LDS, and
// above all the drain of its stores before its LDS can be handed on), and the first version - float32-input MFMA,
// 34.5 KiB of LDS, 4 workgroups per CU - took the same 0.32 ms whether its 2048 matrix-core cycles per block were cut
// to 384, or its stores were rearranged into whole 512-byte runs (a 128 x 64 output-stationary tiling, 1.5 x the
// products, 121 KiB of LDS: 0.40 ms).  So this version is built for a small footprint instead:
//   * operands as two f16 numbers each (x * 2^10 = hi + lo; unit vectors, 22 significand bits), three
//     v_mfma_f32_32x32x16_f16 products per K step (hi*hi + hi*lo + lo*hi), float32 accumulation, 384 matrix-core cycles
//     per block.  Measured against the float64 dot product over every scored entry (tests/test_cost_volume_mfma_gpu.py,
//     profiles/parity_cost_volume_mfma.json): <= 9.4e-8 on independent Gaussian unit vectors (scores near 0), <= 2.5e-7
//     on true matches (fr = +-fl, scores near -+1), <= 3.6e-7 when all components are non-negative - 1.0 to 2.8 times
//     the error NumPy's float32 pairwise sum makes on the same inputs; exact where the scores are exactly representable;
//   * the 64 channels staged in two halves (18 KiB for both operand tiles; the second half waits in registers);
//   * the product tile T diagonal-major but folded: diagonal dd >= 0 (columns dd..63) and diagonal dd - 64 (columns
//     0..dd-1) share row dd of T[64][68] - 17 KiB instead of 34 - and the quads that straddle the fold are the ragged
//     ends of both diagonals, written element by element.
// 18 KiB of LDS: 8 workgroups per CU.  The accumulator is staged through LDS so that stores run along w for fixed d.
using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef _Float16 cv_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 cv_h4 __attribute__((ext_vector_type(4)));
constexpr int CVM_SP = 144;  // LDS bytes per operand pixel and channel half: [K step][hi 32 B | lo 32 B] + 16 pad
constexpr int CVM_TP = 68;   // LDS pitch of the folded product tile T[(w-x) & 63][w] (floats, 16-byte rows)

// v_med3_f32 returns the minimum of the other two operands when one is NaN: the clamp alone would turn a NaN feature
// (mccnn_l2norm_chw_to_hwc keeps one on purpose) into -65504 and its scores into finite numbers.  NaN passes instead,
// through both halves and the matrix cores, and marks every score of its pixel as it does in the exact mode.
__device__ __forceinline__ float cv_scale_clamp(float v)
{
    const float s = v * 1024.f;
    const float c = __builtin_amdgcn_fmed3f(s, -65504.f, 65504.f);
    return s != s ? s : c;
}

__device__ __forceinline__ void cv_split4(const float4 v, cv_h4 &hi, cv_h4 &lo)
{
    // unit vectors never get near the clamp (|x| <= 1 -> 1024); it keeps finite features that are not normalised finite
    const float x[4] = {cv_scale_clamp(v.x), cv_scale_clamp(v.y), cv_scale_clamp(v.z), cv_scale_clamp(v.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const _Float16 h = (_Float16)x[j];
        hi[j] = h;
        lo[j] = (_Float16)(x[j] - (float)h);
    }
}

// PIXEL_MAJOR (round 4): the product tile goes to LDS as it is, T[w][x], and leaves as whole disparity runs of the
// pixel-major volumes "HWD" [H][W][Dp] - a left pixel w takes its row of T (d = w - x: 64 consecutive disparities, 256
// bytes), a right pixel x its column - so that the matrix-core cost volume can feed the pixel-major pipeline without a
// layout change (mccnn_cost_volume_hwd with MCCNN_CV_MFMA).  Same products, same bits as the plane-major form.
template <bool PIXEL_MAJOR>
__global__ __launch_bounds__(256, CVM_WAVES_PER_SIMD) void cost_volume_mfma_kernel(
    const float *__restrict__ fl, const float *__restrict__ fr, int H, int W, int D, float *__restrict__ lcv,
    float *__restrict__ rcv, int nwt, int nbands, int total, int Dp)
{
    // operand tiles (one channel half at a time) and, after the products are done, the folded product tile share one
    // allocation
    constexpr int LDS_BYTES = (2 * 64 * CVM_SP > 64 * CVM_TP * 4) ? 2 * 64 * CVM_SP : 64 * CVM_TP * 4;
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    char *oL = lds, *oR = lds + 64 * CVM_SP;
    float *sT = reinterpret_cast<float *>(lds);
    // tile (bw, bx): left columns w0..w0+63, right columns x0..x0+63; d = w - x in (w0-x0-63 .. w0-x0+63)
    // Work order.  The pieces of one 128-byte line of a volume row come from neighbouring tiles (the next w tile, the
    // next band), and the dispatcher deals consecutive workgroups to the 8 XCDs round-robin - with the plain grid
    // order every L2 ended up holding partial lines and wrote them back partially (the store phase cost 0.28 ms of
    // 0.46).  So the launch is 1-D and each XCD gets a contiguous range of (row, band, w tile) work items: all
    // tiles of an image row meet in one L2 and lines leave it whole.  (Placement only affects speed.)
    int id;
    {
        const int b = blockIdx.x, qq = total >> 3, r = total & 7, xc = b & 7;
        id = (xc < r ? xc * (qq + 1) : r * (qq + 1) + (xc - r) * qq) + (b >> 3);
    }
    const int wt = id % nwt, band = (id / nwt) % nbands;
    const int h = id / (nwt * nbands);
    const int w0 = wt * 64;
    const int x0 = w0 - band * 64;  // band 0 -> x0 = w0, 1 -> x0 = w0-64, ...
    if (x0 + 63 < 0) return;
    if (w0 - x0 - 63 >= D) return;
    const int tid = threadIdx.x;
    const size_t rowbase = (size_t)h * W;
    // piece p = j*256 + tid of a channel half: pixel p >> 3, channels 4 (p & 7) .. + 3 of the half
    float4 vl[2][2], vr[2][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = j * 256 + tid, px = p >> 3, c4 = hf * 8 + (p & 7);
            vl[hf][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            vr[hf][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (w0 + px < W) vl[hf][j] = *reinterpret_cast<const float4 *>(fl + (rowbase + w0 + px) * CV_C + c4 * 4);
            const int x = x0 + px;
            if (x >= 0 && x < W) vr[hf][j] = *reinterpret_cast<const float4 *>(fr + (rowbase + x) * CV_C + c4 * 4);
        }
    const int wave = tid >> 6, lane = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;  // this wave's 32x32 sub-block (w rows, x cols)
    f32x16 acc, acc2;                                       // hi*hi, and the two cross terms
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f, acc2[i] = 0.f;
    const char *pa = oL + (wr + (lane & 31)) * CVM_SP + 16 * (lane >> 5);
    const char *pb = oR + (wc + (lane & 31)) * CVM_SP + 16 * (lane >> 5);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        if (hf) __syncthreads();   // everyone is done with the first half's tiles
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = j * 256 + tid, px = p >> 3, c = p & 7;
            const int off = px * CVM_SP + (c >> 2) * 64 + (c & 3) * 8;
            cv_h4 hh, ll;
            cv_split4(vl[hf][j], hh, ll);
            *reinterpret_cast<cv_h4 *>(oL + off) = hh;
            *reinterpret_cast<cv_h4 *>(oL + off + 32) = ll;
            cv_split4(vr[hf][j], hh, ll);
            *reinterpret_cast<cv_h4 *>(oR + off) = hh;
            *reinterpret_cast<cv_h4 *>(oR + off + 32) = ll;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const cv_h8 a_hi = *reinterpret_cast<const cv_h8 *>(pa + q * 64);
            const cv_h8 a_lo = *reinterpret_cast<const cv_h8 *>(pa + q * 64 + 32);
            const cv_h8 b_hi = *reinterpret_cast<const cv_h8 *>(pb + q * 64);
            const cv_h8 b_lo = *reinterpret_cast<const cv_h8 *>(pb + q * 64 + 32);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc2, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc2, 0, 0, 0);
        }
    }
    __syncthreads();   // every wave is done with the operand tiles: their LDS becomes the product tile
    if (PIXEL_MAJOR) {
        constexpr int TP = 65;
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
            const int row = wr + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);
            const int col = wc + (lane & 31);
            sT[row * TP + col] = (acc[rg] + acc2[rg]) * (-1.f / 1048576.f);
        }
        __syncthreads();
        const int dbase = w0 - x0;
        // left volume: pixel w0 + r takes row r of T: lane = x, d = dbase + r - lane
        for (int r = wave; r < 64; r += 4) {
            const int w = w0 + r, d = dbase + r - lane;
            if (w < W && d >= 0 && d < D && w >= d) lcv[(rowbase + w) * (size_t)Dp + d] = sT[r * TP + lane];
        }
        // right volume: pixel x0 + c takes column c of T: lane = w, d = dbase + lane - c
        for (int c = wave; c < 64; c += 4) {
            const int x = x0 + c, d = dbase + lane - c;
            if (x >= 0 && w0 + lane < W && d >= 0 && d < D) rcv[(rowbase + x) * (size_t)Dp + d] = sT[lane * TP + c];
        }
        return;
    }
    // Products go to LDS diagonal-major and folded, already negated: T[(w - x) & 63][w] (w, x local).  A row of T
    // holds diagonal dd = row in its columns row..63 and diagonal row - 64 in its columns 0..row-1; both run along
    // w, which is how both volumes are written (lcv[d][h][w] and rcv[d][h][w - d]).
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
        const int row = wr + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);
        const int col = wc + (lane & 31);
        sT[((row - col) & 63) * CVM_TP + row] = (acc[rg] + acc2[rg]) * (-1.f / 1048576.f);
    }
    __syncthreads();
    const size_t plane = (size_t)H * W;
    const int dbase = w0 - x0;  // d of the main diagonal
    // A lane stores 4 consecutive w of one diagonal (16 B, dword aligned) to both volumes - the vector-memory pipe
    // costs about the same per wave instruction whatever its width; one instruction covers 4 rows of T x 16 quads.
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const int q = lane & 15, sub = lane >> 4;
    for (int rgp = wave; rgp < 16; rgp += 4) {
        const int row = rgp * 4 + sub;
        const int wl = 4 * q;          // first w_local of this lane's quad
        const float4 t = *reinterpret_cast<const float4 *>(&sT[row * CVM_TP + wl]);
        const float v[4] = {t.x, t.y, t.z, t.w};
        const int w = w0 + wl;
        if (wl >= row || wl + 3 < row) {
            const int dd = wl >= row ? row : row - 64;
            const int d = dbase + dd;
            if (d < 0 || d >= D || w >= W) continue;
            float *pl = lcv + (size_t)d * plane + rowbase + w;
            float *pr = rcv + (size_t)d * plane + rowbase + (w - d);
            if (w + 3 < W) {
                f4u o;
                o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
                *reinterpret_cast<f4u *>(pl) = o;
                *reinterpret_cast<f4u *>(pr) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (w + j < W) {
                        pl[j] = v[j];
                        pr[j] = v[j];
                    }
            }
        }
    }
    // The quad of a row that straddles the fold (rows not divisible by 4) holds the last elements of one diagonal and
    // the first of the other: one element per thread, all lanes busy - 2 store instructions per wave instead of 8
    // nearly empty ones inside every iteration of the loop above.
    {
        const int row = tid >> 2, j = tid & 3;
        const int c = (row & ~3) + j;                     // column of the element in its row of T
        const int d = dbase + (c >= row ? row : row - 64);
        const int w = w0 + c;
        if ((row & 3) != 0 && d >= 0 && d < D && w < W) {
            const float v = sT[row * CVM_TP + c];
            lcv[(size_t)d * plane + rowbase + w] = v;
            rcv[(size_t)d * plane + rowbase + (w - d)] = v;
        }
    }
}

// Border recurrences on the negated volumes.  One wavefront per (plane d, 64 image rows, side): lane = row, each lane
// runs its own 3-tap recurrence (<= d sequential steps); 64 steps are staged in LDS and written back transposed, so the
// stores are 256-byte runs along w instead of 64 scattered dwords per instruction.
__global__ __launch_bounds__(64) void cost_volume_fill_kernel(float *__restrict__ lcv, float *__restrict__ rcv, int D,
                                                              int H, int W)
{
    __shared__ float tile[64 * 65];
    const int lane = threadIdx.x;
    const int d = D - 1 - blockIdx.y;          // plane 0 has no border; the longest recurrences start first
    const int h0 = blockIdx.x * 64;
    const int h = min(h0 + lane, H - 1);       // surplus lanes repeat the last row and store nothing
    const int nrows = min(64, H - h0);
    if (blockIdx.z == 0) {
        // pf:94-95: column w = d-1 .. 0 from columns w+1, w+2, w+3 (NumPy sums them in ascending order)
        float *L = lcv + ((size_t)d * H + h) * W;
        float x1 = L[d], x2 = L[d + 1], x3 = L[d + 2];
        for (int wtop = d - 1; wtop >= 0; wtop -= 64) {
            const int cnt = min(64, wtop + 1);
            for (int j = 0; j < cnt; ++j) {
                // (the reference sums BEFORE it negates, and NumPy's reduction starts from the identity +0: the sum of the
                // reference's values is 0 - x1 - x2 - x3 on the negated ones - the same bits, a zero sum's sign included)
                float s = 0.f - x1;
                s = s - x2;
                s = s - x3;
                const float v = -(s / 3.f);
                tile[lane * 65 + j] = v;
                x3 = x2; x2 = x1; x1 = v;
            }
            __syncthreads();
            if (lane < cnt)
                for (int r = 0; r < nrows; ++r)
                    lcv[((size_t)d * H + h0 + r) * W + (wtop - lane)] = tile[r * 65 + lane];
            __syncthreads();
        }
    } else {
        // pf:105-106: column w = W-d .. W-1 from columns w-3, w-2, w-1
        float *Rr = rcv + ((size_t)d * H + h) * W;
        float x1 = Rr[W - d - 3], x2 = Rr[W - d - 2], x3 = Rr[W - d - 1];
        for (int wbot = W - d; wbot < W; wbot += 64) {
            const int cnt = min(64, W - wbot);
            for (int j = 0; j < cnt; ++j) {
                // (the reference sums BEFORE it negates, and NumPy's reduction starts from the identity +0: the sum of the
                // reference's values is 0 - x1 - x2 - x3 on the negated ones - the same bits, a zero sum's sign included)
                float s = 0.f - x1;
                s = s - x2;
                s = s - x3;
                const float v = -(s / 3.f);
                tile[lane * 65 + j] = v;
                x1 = x2; x2 = x3; x3 = v;
            }
            __syncthreads();
            if (lane < cnt)
                for (int r = 0; r < nrows; ++r)
                    rcv[((size_t)d * H + h0 + r) * W + (wbot + lane)] = tile[r * 65 + lane];
            __syncthreads();
        }
    }
}

// Border recurrences (pf:94-95, 105-106) on pixel-major volumes: disparities on lanes (4 per lane and 256-group), one
// wave per image row and side, sweeping the columns the borders touch.  Left volume: columns D+1 down to 0; a lane's
// component d takes the stored score while column >= d (those are its three seeds when the sweep reaches d+2, d+1, d)
// and the 3-tap mean of its last three values below that - the same float32 operations in the same order as the
// plane-major fill kernel (NumPy sums the slice in ascending column order: nearest column first here, oldest first on
// the right-volume side).  Right volume: columns W-D-2 up to W-1, scores while column < W - d.
typedef uint32_t cv_u32x4 __attribute__((ext_vector_type(4)));
template <int NG>
__global__ __launch_bounds__(64) void cost_volume_fill_hwd_kernel(float *__restrict__ lcv, float *__restrict__ rcv, int D,
                                                                  int Dp, int H, int W)
{
    constexpr int PF = 8;
    constexpr int kDrop = 0x7ffffff0;
    const int lane = threadIdx.x, h = blockIdx.x;
    const bool left = blockIdx.y == 0;
    float *row = (left ? lcv : rcv) + (size_t)h * W * Dp;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, (int)((size_t)W * Dp * 4), 0x00020000);
    const unsigned pix = (unsigned)Dp * 4u;
    const int c_first = left ? D + 1 : max(W - D - 2, 0), nsteps = left ? D + 2 : W - c_first;
    auto col = [&](int t) { return left ? c_first - t : c_first + t; };
    int dbase[NG], voff[NG];
    float x1[NG][4], x2[NG][4], x3[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        dbase[g] = g * 256 + lane * 4;
        voff[g] = dbase[g] < Dp ? dbase[g] * 4 : kDrop;
#pragma unroll
        for (int i = 0; i < 4; ++i) x1[g][i] = x2[g][i] = x3[g][i] = 0.f;
    }
    cv_u32x4 buf[PF][NG];
    auto issue = [&](int slot, int t) {
        const unsigned so = (unsigned)col(min(t, nsteps - 1)) * pix;
#pragma unroll
        for (int g = 0; g < NG; ++g) buf[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[g], so, 0);
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) issue(k, k);
    for (int t0 = 0; t0 < nsteps; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            if (t >= nsteps) continue;
            const int c = col(t);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const cv_u32x4 u = buf[k][g];
                const float v[4] = {__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
                cv_u32x4 o;
                bool any = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = dbase[g] + i;
                    const bool stored = left ? c >= d : c < W - d;     // the score itself (d >= D: pad, never used)
                    float s = 0.f - x1[g][i];     // the reference's (0 + x1 + x2 + x3) / 3 on its not yet negated values
                    s = s - x2[g][i];
                    s = s - x3[g][i];
                    const float val = stored ? v[i] : -(s / 3.f);
                    any |= !stored && d < D;
                    if (left) { x3[g][i] = x2[g][i]; x2[g][i] = x1[g][i]; x1[g][i] = val; }     // x1 = column c + 1 next
                    else      { x1[g][i] = x2[g][i]; x2[g][i] = x3[g][i]; x3[g][i] = val; }     // x3 = column c - 1 next
                    o[i] = __float_as_uint(val);
                }
                // components that still hold their score are written back unchanged
                buffer_store_b128<0>(o, rs, any ? voff[g] : kDrop, (unsigned)c * pix);
            }
            issue(k, t + PF);
        }
    }
}


// The same recurrences with ONE disparity per lane: a wave owns 64 consecutive disparities of one image row and side,
// so a row has Dp / 64 waves instead of one (cfg2: 4000 waves instead of 1000 - the four-per-lane form above is one
// wave per SIMD walking D + 2 dependent 1 KiB loads, 0.13 ms of latency for 34 M entries), each sweeping only the
// columns its own disparities touch (chunk q: 64 q + 66 of them), 16 loads in flight.  Same float32 operations in the
// same order per entry as cost_volume_fill_hwd_kernel (and as the plane-major fill kernel): bit-identical.
__global__ __launch_bounds__(64) void cost_volume_fill_hwd_lanes_kernel(float *__restrict__ lcv, float *__restrict__ rcv,
                                                                        int D, int Dp, int H, int W)
{
    constexpr int PF = 16;
    constexpr int kDrop = 0x7ffffff0;
    const int lane = threadIdx.x, h = blockIdx.x;
    const bool left = blockIdx.y == 0;
    const int d = (int)blockIdx.z * 64 + lane;
    const int dmax = min((int)blockIdx.z * 64 + 63, D - 1);       // the largest disparity of this wave that exists
    if ((int)blockIdx.z * 64 >= D) return;
    float *row = (left ? lcv : rcv) + (size_t)h * W * Dp;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, (int)((size_t)W * Dp * 4), 0x00020000);
    const unsigned pix = (unsigned)Dp * 4u;
    const int c_first = left ? dmax + 2 : max(W - dmax - 3, 0), nsteps = left ? c_first + 1 : W - c_first;
    auto col = [&](int t) { return left ? c_first - t : c_first + t; };
    const int voff = d < Dp ? d * 4 : kDrop;
    const int sto = d < D ? voff : kDrop;
    float x1 = 0.f, x2 = 0.f, x3 = 0.f;
    float buf[PF];
    // Phase A: the columns from which some lane of the wave still takes its score (columns >= the wave's smallest
    // disparity on the left side, < W - that disparity on the right): at most 66 of them.  Their loads are
    // unconditional (a step past the last such column re-reads it, unused), so the compiler's vmcnt bookkeeping stays
    // exact - a load inside a condition made every step wait for everything in flight, its own store included.
    const int dmin = (int)blockIdx.z * 64;
    const int nA = min(nsteps, left ? c_first - dmin + 1 : (W - dmin) - c_first);
    auto issue = [&](int slot, int t) {
        const int c = col(min(t, nA - 1));
        buf[slot] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (unsigned)c * pix, 0));
    };
    // s / 3.f, correctly rounded, in three operations instead of the compiler's ten: q = RN(s * RN(1/3)), one residual,
    // one correction (division by a constant, Brisebarre / Muller).  tools/probe/div3_exhaustive.c compares it with the
    // division for ALL 2^32 float32 inputs: identical bits (denormals, NaN payloads included) except for -0.0 and
    // +-inf, which are handed through as they are (s / 3 = s for them).  The recurrence is a chain of 250 dependent
    // steps per wave with four waves per SIMD: the division was most of its time.
    auto third = [](float s) {
        const float zh = 0.3333333432674407958984375f;            // RN(1/3) = 0x3eaaaaab
        const float q = s * zh;
        const float r = __builtin_fmaf(-3.0f, q, s);
        const float q2 = __builtin_fmaf(r, zh, q);
        return (__builtin_fabsf(s) < __builtin_inff() && s != 0.f) ? q2 : s;
    };
    auto step = [&](int c, bool stored, float have) {
        // the reference's (0 + x1 + x2 + x3) / 3 on its not yet negated values (pf:94-95 run before pf:111-112, and NumPy's
        // reduction starts from the identity +0): 0 - x1 - x2 - x3 on the negated ones, negated again - the same bits as
        // summing the stored values except that a sum that is exactly zero comes out as -0.0, like the reference's
        float s = 0.f - x1;
        s = s - x2;
        s = s - x3;
        const float val = stored ? have : -third(s);
        if (left) { x3 = x2; x2 = x1; x1 = val; }               // x1 = column c + 1 next
        else      { x1 = x2; x2 = x3; x3 = val; }               // x3 = column c - 1 next
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), rs, stored ? kDrop : sto, (unsigned)c * pix, 0);
    };
    if (nA > 0) {
#pragma unroll
        for (int k = 0; k < PF; ++k) issue(k, k);
        for (int t0 = 0; t0 < nA; t0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const int t = t0 + k;
                if (t < nA) {
                    const int c = col(t);
                    step(c, left ? c >= d : c < W - d, buf[k]);     // stored: the score itself (d >= D: pad, never used)
                }
                issue(k, t + PF);
            }
        }
    }
    // Phase B: behind them the sweep is pure recurrence for every lane - no load, hence no wait: the stores just leave
    for (int t = max(nA, 0); t < nsteps; ++t) step(col(t), false, 0.f);
}

// The border recurrences as launches of their own: every producer of the w >= d scores (the feature dot products here,
// the decision network of decision_mfma.hip) ends with them.
int launch_cost_volume_fill(float *lcv, float *rcv, int D, int H, int W, hipStream_t s, const char *what)
{
    if (D > 1)
        hipLaunchKernelGGL(cost_volume_fill_kernel, dim3(cdiv(H, 64), D - 1, 2), dim3(64), 0, s, lcv, rcv, D, H, W);
    return check_launch(what);
}

int launch_cost_volume_fill_hwd(float *lcv_hwd, float *rcv_hwd, int D, int Dp, int H, int W, hipStream_t s, const char *what)
{
    if (D > 1) {
#ifdef CV_FILL_FOUR_PER_LANE     // A/B builds: the four-disparities-per-lane sweep (one wave per row and side)
        if (Dp <= 256)
            hipLaunchKernelGGL(cost_volume_fill_hwd_kernel<1>, dim3(H, 2), dim3(64), 0, s, lcv_hwd, rcv_hwd, D, Dp, H, W);
        else
            hipLaunchKernelGGL(cost_volume_fill_hwd_kernel<2>, dim3(H, 2), dim3(64), 0, s, lcv_hwd, rcv_hwd, D, Dp, H, W);
#else
        hipLaunchKernelGGL(cost_volume_fill_hwd_lanes_kernel, dim3(H, 2, cdiv(D, 64)), dim3(64), 0, s, lcv_hwd, rcv_hwd, D, Dp,
                           H, W);
#endif
    }
    return check_launch(what);
}

}  // namespace mccnn

extern "C" int mccnn_cost_volume(const float *fl, const float *fr, int H, int W, int C, int D, float *lcv, float *rcv,
                                 int mode, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(fl && fr && lcv && rcv, MCCNN_E_INVALID, "mccnn_cost_volume: null pointer");
    MCCNN_REQUIRE(H > 0 && W > 0 && D > 0, MCCNN_E_INVALID, "mccnn_cost_volume: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume: D=%d needs W >= D+2 (the reference's border recurrence pf:106 is degenerate "
                  "beyond that), W=%d", D, W);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    if (mode == MCCNN_CV_EXACT) {
        const dim3 grid(cdiv(W, CV_TW), H, cdiv(D, CV_DT));
        hipLaunchKernelGGL(cost_volume_exact_kernel<false>, grid, block, 0, s, fl, fr, H, W, D, lcv, rcv, 0);
    } else if (mode == MCCNN_CV_MFMA) {
        const int nwt = cdiv(W, 64), nbands = cdiv(D + 63, 64) + 1;
        const long total = (long)nwt * nbands * H;
        MCCNN_REQUIRE(total <= 0x7fffffffL, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume: %ld tiles exceed the grid", total);
        hipLaunchKernelGGL(cost_volume_mfma_kernel<false>, dim3((unsigned)total), block, 0, s, fl, fr, H, W, D, lcv, rcv, nwt,
                           nbands, (int)total, 0);
    } else {
        MCCNN_REQUIRE(false, MCCNN_E_INVALID, "mccnn_cost_volume: unknown mode %d", mode);
    }
    int rc = check_launch("mccnn_cost_volume");
    if (rc) return rc;
    return launch_cost_volume_fill(lcv, rcv, D, H, W, s, "mccnn_cost_volume(fill)");
}

extern "C" int mccnn_cost_volume_hwd(const float *fl, const float *fr, int H, int W, int C, int D, float *lcv_hwd,
                                     float *rcv_hwd, int mode, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(fl && fr && lcv_hwd && rcv_hwd, MCCNN_E_INVALID, "mccnn_cost_volume_hwd: null pointer");
    MCCNN_REQUIRE(H > 0 && W > 0 && D > 0, MCCNN_E_INVALID, "mccnn_cost_volume_hwd: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_hwd: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_hwd: D=%d needs W >= D+2 (the reference's border recurrence pf:106 is degenerate "
                  "beyond that), W=%d", D, W);
    MCCNN_REQUIRE(mode == MCCNN_CV_EXACT || mode == MCCNN_CV_MFMA, MCCNN_E_INVALID, "mccnn_cost_volume_hwd: unknown mode %d",
                  mode);
#ifdef CV_FILL_FOUR_PER_LANE     // (its sweep holds at most two 256-disparity groups)
    constexpr int kMaxD = 512;
#else                            // the product kernels walk 64-disparity tiles, the fill kernel 64-disparity waves
    constexpr int kMaxD = 1024;
#endif
    MCCNN_REQUIRE(D <= kMaxD, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_hwd: D=%d > %d", D, kMaxD);
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_hwd: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    hipStream_t s = (hipStream_t)stream;
    if (mode == MCCNN_CV_MFMA) {
        const int nwt = cdiv(W, 64), nbands = cdiv(D + 63, 64) + 1;
        const long total = (long)nwt * nbands * H;
        MCCNN_REQUIRE(total <= 0x7fffffffL, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_hwd: %ld tiles exceed the grid", total);
        hipLaunchKernelGGL(cost_volume_mfma_kernel<true>, dim3((unsigned)total), dim3(256), 0, s, fl, fr, H, W, D, lcv_hwd,
                           rcv_hwd, nwt, nbands, (int)total, Dp);
    } else {
#ifdef CV_HWD_TILE_KERNEL      // A/B builds: one LDS row per score
        const dim3 grid(cdiv(W, CV_TW), H, cdiv(D, CV_DT));
        hipLaunchKernelGGL(cost_volume_exact_kernel<true>, grid, dim3(256), 0, s, fl, fr, H, W, D, lcv_hwd, rcv_hwd, Dp);
#else
        const dim3 grid(cdiv(W, CVP_TW), H, 1);
        hipLaunchKernelGGL(cost_volume_exact_pairs_kernel, grid, dim3(256), 0, s, fl, fr, H, W, D, lcv_hwd, rcv_hwd, Dp);
#endif
    }
    int rc = check_launch("mccnn_cost_volume_hwd");
    if (rc) return rc;
    return launch_cost_volume_fill_hwd(lcv_hwd, rcv_hwd, D, Dp, H, W, s, "mccnn_cost_volume_hwd(fill)");
}

extern "C" int mccnn_cost_volume_vertical_hwd(const float *fl, const float *fr, int H, int W, int C, int D,
                                              int vertical_range, float *lcv_hwd, float *rcv_hwd, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(fl && fr && lcv_hwd && rcv_hwd, MCCNN_E_INVALID, "mccnn_cost_volume_vertical_hwd: null pointer");
    MCCNN_REQUIRE(vertical_range >= 0 && vertical_range <= MCCNN_VERTICAL_RANGE_MAX, MCCNN_E_INVALID,
                  "mccnn_cost_volume_vertical_hwd: vertical_range=%d outside [0, %d]", vertical_range,
                  MCCNN_VERTICAL_RANGE_MAX);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "mccnn_cost_volume_vertical_hwd: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_vertical_hwd: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D >= 2 && D <= 1024, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_vertical_hwd: D=%d outside [2, 1024]", D);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_vertical_hwd: D=%d needs W >= D+2 (the reference's border recurrence pf:106 is "
                  "degenerate beyond that), W=%d", D, W);
    MCCNN_REQUIRE(H <= 65535, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_vertical_hwd: H=%d > 65535 rows exceed the grid", H);
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_vertical_hwd: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(W, CVP_TW), H, 1);
    if (vertical_range == 0)      // one candidate: both volumes out of the same products (pf:104), the pairs kernel as it is
        hipLaunchKernelGGL(cost_volume_exact_pairs_kernel, grid, dim3(256), 0, s, fl, fr, H, W, D, lcv_hwd, rcv_hwd, Dp);
    else
        hipLaunchKernelGGL(cost_volume_vertical_kernel<false>, dim3(grid.x, grid.y, 2), dim3(256), 0, s, fl, fr, H, W, D,
                           vertical_range, lcv_hwd, rcv_hwd, Dp, (const int *)nullptr);
    int rc = check_launch("mccnn_cost_volume_vertical_hwd");
    if (rc) return rc;
    return launch_cost_volume_fill_hwd(lcv_hwd, rcv_hwd, D, Dp, H, W, s, "mccnn_cost_volume_vertical_hwd(fill)");
}

extern "C" int mccnn_cost_volume_offset_hwd(const float *fl, const float *fr, int H, int W, int C, int D,
                                            const int32_t *row_offset, int vertical_range, float *lcv_hwd, float *rcv_hwd,
                                            mccnn_stream_t stream)
{
    using namespace mccnn;
    if (!row_offset)              // offset 0: the search as it is, the same launches
        return mccnn_cost_volume_vertical_hwd(fl, fr, H, W, C, D, vertical_range, lcv_hwd, rcv_hwd, stream);
    MCCNN_REQUIRE(fl && fr && lcv_hwd && rcv_hwd, MCCNN_E_INVALID, "mccnn_cost_volume_offset_hwd: null pointer");
    MCCNN_REQUIRE(vertical_range >= 0 && vertical_range <= MCCNN_VERTICAL_RANGE_MAX, MCCNN_E_INVALID,
                  "mccnn_cost_volume_offset_hwd: vertical_range=%d outside [0, %d]", vertical_range, MCCNN_VERTICAL_RANGE_MAX);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "mccnn_cost_volume_offset_hwd: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_offset_hwd: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D >= 2 && D <= 1024, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_offset_hwd: D=%d outside [2, 1024]", D);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_offset_hwd: D=%d needs W >= D+2 (the reference's border recurrence pf:106 is "
                  "degenerate beyond that), W=%d", D, W);
    MCCNN_REQUIRE(H <= 65535, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_offset_hwd: H=%d > 65535 rows exceed the grid", H);
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_offset_hwd: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    hipStream_t s = (hipStream_t)stream;
    // (range 0: one candidate per view, two product sets - the offset is known on the device only, so the pairs kernel,
    // whose two volumes share their products, cannot serve it)
    hipLaunchKernelGGL(cost_volume_vertical_kernel<true>, dim3(cdiv(W, CVP_TW), H, 2), dim3(256), 0, s, fl, fr, H, W, D,
                       vertical_range, lcv_hwd, rcv_hwd, Dp, (const int *)row_offset);
    int rc = check_launch("mccnn_cost_volume_offset_hwd");
    if (rc) return rc;
    return launch_cost_volume_fill_hwd(lcv_hwd, rcv_hwd, D, Dp, H, W, s, "mccnn_cost_volume_offset_hwd(fill)");
}

extern "C" int mccnn_vertical_profile_rows(int H, int row_step)
{
    if (H <= 0 || row_step < 1 || row_step / 2 >= H) return 0;
    return (H - 1 - row_step / 2) / row_step + 1;
}

extern "C" int mccnn_vertical_profile(const float *fl, const float *fr, int H, int W, int C, int D, int max_offset,
                                      int row_step, uint32_t *votes, size_t votes_bytes, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(fl && fr, MCCNN_E_INVALID, "mccnn_vertical_profile: null pointer");
    MCCNN_REQUIRE(max_offset >= 0 && max_offset <= MCCNN_VERTICAL_OFFSET_MAX, MCCNN_E_INVALID,
                  "mccnn_vertical_profile: max_offset=%d outside [0, %d]", max_offset, MCCNN_VERTICAL_OFFSET_MAX);
    MCCNN_REQUIRE(row_step >= 1, MCCNN_E_INVALID, "mccnn_vertical_profile: row_step=%d < 1", row_step);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "mccnn_vertical_profile: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_vertical_profile: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D >= 2 && D <= 1024, MCCNN_E_UNSUPPORTED, "mccnn_vertical_profile: D=%d outside [2, 1024]", D);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED, "mccnn_vertical_profile: D=%d needs W >= D+2, W=%d", D, W);
    MCCNN_REQUIRE(H <= 65535, MCCNN_E_UNSUPPORTED, "mccnn_vertical_profile: H=%d > 65535 rows exceed the grid", H);
    MCCNN_REQUIRE((size_t)W * mccnn_hwd_pitch(D) * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_vertical_profile: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    const int n_rows = mccnn_vertical_profile_rows(H, row_step), n_blocks = cdiv(W, 64);
    const size_t need = (size_t)n_rows * n_blocks * (2 * max_offset + 1) * sizeof(uint32_t);
    MCCNN_REQUIRE(votes_bytes >= need, MCCNN_E_SCRATCH, "mccnn_vertical_profile: the votes need %zu bytes, %zu given", need,
                  votes_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) return 0;                       // row_step / 2 >= H: no profiled row, no vote, an empty array
    MCCNN_REQUIRE(votes, MCCNN_E_INVALID, "mccnn_vertical_profile: null pointer");
    MCCNN_REQUIRE(hipMemsetAsync(votes, 0, need, s) == hipSuccess, MCCNN_E_INVALID, "mccnn_vertical_profile: memset failed");
    hipLaunchKernelGGL(vertical_profile_kernel, dim3(cdiv(W, CVP_TW), n_rows, 1), dim3(256), 0, s, fl, fr, H, W, D, max_offset,
                       row_step, votes, n_blocks);
    return check_launch("mccnn_vertical_profile");
}

extern "C" int mccnn_vertical_offset_select(const uint32_t *votes, int n_rows, int n_blocks, int max_offset, int32_t *offset,
                                            uint64_t *totals, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(offset && totals, MCCNN_E_INVALID, "mccnn_vertical_offset_select: null pointer");
    MCCNN_REQUIRE(max_offset >= 0 && max_offset <= MCCNN_VERTICAL_OFFSET_MAX, MCCNN_E_INVALID,
                  "mccnn_vertical_offset_select: max_offset=%d outside [0, %d]", max_offset, MCCNN_VERTICAL_OFFSET_MAX);
    MCCNN_REQUIRE(n_rows >= 0 && n_blocks >= 0 && (long)n_rows * n_blocks <= 0x7fffffffL, MCCNN_E_INVALID,
                  "mccnn_vertical_offset_select: %d rows x %d blocks", n_rows, n_blocks);
    // (an empty array - no profiled row - has no address: nothing is read, the offset is 0)
    MCCNN_REQUIRE(votes || (long)n_rows * n_blocks == 0, MCCNN_E_INVALID, "mccnn_vertical_offset_select: null pointer");
    hipLaunchKernelGGL(vertical_offset_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, votes, n_rows * n_blocks,
                       max_offset, offset, reinterpret_cast<unsigned long long *>(totals));
    return check_launch("mccnn_vertical_offset_select");
}

extern "C" int mccnn_vertical_field_select(const uint32_t *votes, int n_rows, int n_blocks, int H, int row_step,
                                           int max_offset, int gh, int gw, int32_t *field, uint64_t *totals, int32_t *offset,
                                           uint64_t *global_totals, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(field && totals && offset && global_totals, MCCNN_E_INVALID, "mccnn_vertical_field_select: null pointer");
    MCCNN_REQUIRE(max_offset >= 0 && max_offset <= MCCNN_VERTICAL_OFFSET_MAX, MCCNN_E_INVALID,
                  "mccnn_vertical_field_select: max_offset=%d outside [0, %d]", max_offset, MCCNN_VERTICAL_OFFSET_MAX);
    MCCNN_REQUIRE(H > 0, MCCNN_E_INVALID, "mccnn_vertical_field_select: H=%d is not positive", H);
    MCCNN_REQUIRE(row_step >= 1, MCCNN_E_INVALID, "mccnn_vertical_field_select: row_step=%d < 1", row_step);
    MCCNN_REQUIRE(n_rows == mccnn_vertical_profile_rows(H, row_step), MCCNN_E_INVALID,
                  "mccnn_vertical_field_select: n_rows=%d, but H=%d at row_step=%d profiles %d rows", n_rows, H, row_step,
                  mccnn_vertical_profile_rows(H, row_step));
    MCCNN_REQUIRE(n_blocks >= 1 && (long)n_rows * n_blocks <= 0x7fffffffL, MCCNN_E_INVALID,
                  "mccnn_vertical_field_select: %d rows x n_blocks=%d", n_rows, n_blocks);
    MCCNN_REQUIRE(gh >= 1 && gh <= MCCNN_VERTICAL_FIELD_MAX, MCCNN_E_INVALID,
                  "mccnn_vertical_field_select: gh=%d outside [1, %d]", gh, MCCNN_VERTICAL_FIELD_MAX);
    MCCNN_REQUIRE(gw >= 1 && gw <= MCCNN_VERTICAL_FIELD_MAX, MCCNN_E_INVALID,
                  "mccnn_vertical_field_select: gw=%d outside [1, %d]", gw, MCCNN_VERTICAL_FIELD_MAX);
    MCCNN_REQUIRE(gh <= H, MCCNN_E_INVALID, "mccnn_vertical_field_select: gh=%d exceeds the H=%d rows", gh, H);
    MCCNN_REQUIRE(gw <= n_blocks, MCCNN_E_INVALID, "mccnn_vertical_field_select: gw=%d exceeds the n_blocks=%d blocks", gw,
                  n_blocks);
    // (no profiled row: an empty array has no address - nothing is read, every cell takes 0)
    MCCNN_REQUIRE(votes || n_rows == 0, MCCNN_E_INVALID, "mccnn_vertical_field_select: null pointer");
    hipLaunchKernelGGL(vertical_field_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, votes, n_rows, n_blocks, H,
                       row_step, max_offset, gh, gw, field, reinterpret_cast<unsigned long long *>(totals), offset,
                       reinterpret_cast<unsigned long long *>(global_totals));
    return check_launch("mccnn_vertical_field_select");
}

extern "C" int mccnn_cost_volume_field_hwd(const float *fl, const float *fr, int H, int W, int C, int D, const int32_t *field,
                                           int gh, int gw, int vertical_range, float *lcv_hwd, float *rcv_hwd,
                                           mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(fl && fr && field && lcv_hwd && rcv_hwd, MCCNN_E_INVALID, "mccnn_cost_volume_field_hwd: null pointer");
    MCCNN_REQUIRE(vertical_range >= 0 && vertical_range <= MCCNN_VERTICAL_RANGE_MAX, MCCNN_E_INVALID,
                  "mccnn_cost_volume_field_hwd: vertical_range=%d outside [0, %d]", vertical_range, MCCNN_VERTICAL_RANGE_MAX);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "mccnn_cost_volume_field_hwd: non-positive size");
    MCCNN_REQUIRE(C == CV_C, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_field_hwd: C=%d, kernels are built for 64 channels", C);
    MCCNN_REQUIRE(D >= 2 && D <= 1024, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_field_hwd: D=%d outside [2, 1024]", D);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_field_hwd: D=%d needs W >= D+2 (the reference's border recurrence pf:106 is "
                  "degenerate beyond that), W=%d", D, W);
    MCCNN_REQUIRE(H <= 65535, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_field_hwd: H=%d > 65535 rows exceed the grid", H);
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_field_hwd: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    MCCNN_REQUIRE(gh >= 1 && gh <= MCCNN_VERTICAL_FIELD_MAX, MCCNN_E_INVALID,
                  "mccnn_cost_volume_field_hwd: gh=%d outside [1, %d]", gh, MCCNN_VERTICAL_FIELD_MAX);
    MCCNN_REQUIRE(gw >= 1 && gw <= MCCNN_VERTICAL_FIELD_MAX, MCCNN_E_INVALID,
                  "mccnn_cost_volume_field_hwd: gw=%d outside [1, %d]", gw, MCCNN_VERTICAL_FIELD_MAX);
    MCCNN_REQUIRE(gh <= H, MCCNN_E_INVALID, "mccnn_cost_volume_field_hwd: gh=%d exceeds the H=%d rows", gh, H);
    MCCNN_REQUIRE(gw <= cdiv(W, 64), MCCNN_E_INVALID, "mccnn_cost_volume_field_hwd: gw=%d exceeds the %d blocks of W=%d", gw,
                  cdiv(W, 64), W);
    hipStream_t s = (hipStream_t)stream;
    // (the grid travels in the range's argument, so the shipped instantiations keep their signature and their code)
    hipLaunchKernelGGL((cost_volume_vertical_kernel<false, true>), dim3(cdiv(W, CVP_TW), H, 2), dim3(256), 0, s, fl, fr, H, W,
                       D, vertical_range | gh << 8 | gw << 16, lcv_hwd, rcv_hwd, Dp, (const int *)field);
    int rc = check_launch("mccnn_cost_volume_field_hwd");
    if (rc) return rc;
    return launch_cost_volume_fill_hwd(lcv_hwd, rcv_hwd, D, Dp, H, W, s, "mccnn_cost_volume_field_hwd(fill)");
}

extern "C" int mccnn_cost_volume_fill(float *lcv, float *rcv, int D, int H, int W, int pixel_major, mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(lcv && rcv, MCCNN_E_INVALID, "mccnn_cost_volume_fill: null pointer");
    MCCNN_REQUIRE(H > 0 && W > 0 && D > 0, MCCNN_E_INVALID, "mccnn_cost_volume_fill: non-positive size");
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_fill: D=%d needs W >= D+2, W=%d", D, W);
    if (!pixel_major) return launch_cost_volume_fill(lcv, rcv, D, H, W, (hipStream_t)stream, "mccnn_cost_volume_fill");
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE(D <= 1024, MCCNN_E_UNSUPPORTED, "mccnn_cost_volume_fill: D=%d > 1024", D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_fill: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    return launch_cost_volume_fill_hwd(lcv, rcv, D, Dp, H, W, (hipStream_t)stream, "mccnn_cost_volume_fill");
}
