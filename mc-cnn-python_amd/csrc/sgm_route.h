// Which sgm_pass_kernel<NG, PF, FULL, VPL, FAR, ACC> (csrc/sgm.hip) serves a disparity count, and how many steps it keeps
// in flight: the one statement of both rules.  Plain C++ (no HIP), so that a host compiler can check it on its own.
#pragma once
#include <stdint.h>

namespace mccnn {

// ng: groups of 64 * vpl disparities per lane; full: every lane of every group holds vpl real disparities (no tail
// masking); vpl: disparities per lane; far: the rebasing kernels for scanlines beyond one descriptor's 4 GiB reach.
struct SgmRoute { int ng; bool full; int vpl; bool far; };

// far_volume: vertical scanlines (rh != 0) of a volume with H*W*Dp*4 >= 2^32.  One group per 256 disparities, four per
// lane.  The exception: 129 .. 192 disparities whose padded count is a multiple of 3 run three per lane (KITTI's
// D = 192 then fills all 64 lanes, with no tail masks, instead of 48) - on near volumes only, the far kernels are
// four-per-lane throughout.
constexpr SgmRoute sgm_route(int D, bool far_volume)
{
    const int Dp = (D + 3) & ~3;   // mccnn_hwd_pitch
    const int ng = (Dp + 255) / 256;
    const int vpl = (!far_volume && D > 128 && D <= 192 && Dp % 3 == 0) ? 3 : 4;
    return SgmRoute{ng, D == 64 * vpl * ng, vpl, far_volume};
}

// Steps in flight; every entry can be overridden with -D (the tuning tools do).
//
// In place (acc = 0) and the accumulating store form (acc = 1, which holds what the in-place kernel holds): 8, 12 and 16
// measure the same at 750x500x256 (0.30 / 0.29 ms per pass: 1000-1500 scanline waves); a 1242x375 pair has only 750 row
// scanlines - fewer waves than SIMDs - and its horizontal passes gain from 24 steps (0.388 -> 0.342 ms); two disparity
// groups per lane (D > 256) take 12 (vertical 2.17 -> 2.06 ms at 1500x1000x400).
#ifndef SGM_PF_FULL
#define SGM_PF_FULL 16
#endif
#ifndef SGM_PF_PARTIAL
#define SGM_PF_PARTIAL 24
#endif
#ifndef SGM_PF_2G
#define SGM_PF_2G 12
#endif
// Three and four groups (512 < D <= 1024): the step buffers cost 5 VGPRs per group and step (a 16-byte vector + the
// packed flags), so 24 group-steps in flight - the 2 x 12 of two groups - hold the kernels at 3 waves per SIMD
// (<= 168 VGPRs by the register-file table of the MI355X): 3 x 8 -> 160 VGPRs, 4 x 6 -> 168.  One more step (3 x 9, 4 x 7)
// needs 176 / 189 and drops to 2 waves.  Unmeasured: chosen from the register budget alone.
#ifndef SGM_PF_3G
#define SGM_PF_3G 8
#endif
#ifndef SGM_PF_4G
#define SGM_PF_4G 6
#endif
// The accumulating add form (acc = 2) holds one more 16-byte vector per group and step and runs at two thirds of those
// depths (three quarters at D = 256): at least as many 16-byte loads in flight per wave as the in-place kernel has, no
// scratch, 2-3 waves per SIMD by -Rpass-analysis=kernel-resource-usage (the table in DESIGN 4.1).
#ifndef SGM_ACC_PF_FULL
#define SGM_ACC_PF_FULL 12
#endif
#ifndef SGM_ACC_PF_PARTIAL
#define SGM_ACC_PF_PARTIAL 16
#endif
#ifndef SGM_ACC_PF_2G
#define SGM_ACC_PF_2G 8
#endif
#ifndef SGM_ACC_PF_3G
#define SGM_ACC_PF_3G 5
#endif
#ifndef SGM_ACC_PF_4G
#define SGM_ACC_PF_4G 4
#endif

// acc: 0 in place, 1 store, 2 add (sgm_pass_kernel's ACC); column 0: one full group of four per lane (D = 256)
constexpr int kSgmSteps[2][5] = {{SGM_PF_FULL, SGM_PF_PARTIAL, SGM_PF_2G, SGM_PF_3G, SGM_PF_4G},
                                 {SGM_ACC_PF_FULL, SGM_ACC_PF_PARTIAL, SGM_ACC_PF_2G, SGM_ACC_PF_3G, SGM_ACC_PF_4G}};
constexpr int sgm_steps_in_flight(int ng, bool full, int vpl, int acc)
{
    return kSgmSteps[acc == 2][ng == 1 && full && vpl == 4 ? 0 : ng];
}

// The boundaries of the route table, pinned: near volumes, then far ones.
constexpr bool sgm_route_is(int D, bool far_volume, int ng, bool full, int vpl)
{
    const SgmRoute r = sgm_route(D, far_volume);
    return r.ng == ng && r.full == full && r.vpl == vpl && r.far == far_volume;
}
#define SGM_NEAR(D, ng, full, vpl) static_assert(sgm_route_is(D, false, ng, full, vpl), "near route of D = " #D)
#define SGM_FAR(D, ng, full) static_assert(sgm_route_is(D, true, ng, full, 4), "far route of D = " #D)
SGM_NEAR(2, 1, false, 4); SGM_NEAR(128, 1, false, 4); SGM_NEAR(129, 1, false, 3); SGM_NEAR(130, 1, false, 3);
SGM_NEAR(131, 1, false, 3); SGM_NEAR(133, 1, false, 4); SGM_NEAR(191, 1, false, 3); SGM_NEAR(192, 1, true, 3);
SGM_NEAR(193, 1, false, 4); SGM_NEAR(255, 1, false, 4); SGM_NEAR(256, 1, true, 4); SGM_NEAR(257, 2, false, 4);
SGM_NEAR(511, 2, false, 4); SGM_NEAR(512, 2, true, 4); SGM_NEAR(513, 3, false, 4); SGM_NEAR(767, 3, false, 4);
SGM_NEAR(768, 3, true, 4); SGM_NEAR(769, 4, false, 4); SGM_NEAR(1023, 4, false, 4); SGM_NEAR(1024, 4, true, 4);
SGM_FAR(192, 1, false); SGM_FAR(255, 1, false); SGM_FAR(256, 1, true); SGM_FAR(257, 2, false);
SGM_FAR(512, 2, true); SGM_FAR(768, 3, true); SGM_FAR(1000, 4, false); SGM_FAR(1024, 4, true);
#undef SGM_NEAR
#undef SGM_FAR

}  // namespace mccnn
