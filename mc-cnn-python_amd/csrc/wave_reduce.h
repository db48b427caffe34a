// Wave-wide minimum reductions on gfx950 (DPP row operations + two row broadcasts, the result read from lane 63): what
// the winner-take-all kernels (cbca_hwd.hip) and the confidence kernel (confidence.hip) reduce their per-lane candidates
// with.  One copy of the DPP control codes.
#pragma once
#include "common.h"

namespace mccnn {

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ float wave_min_f(float x)
{
    // lanes without a source keep their own value (old = x)
    auto step = [](float v, int o) { return fminf(v, __int_as_float(o)); };
    x = step(x, dpp_i<0xB1>(__float_as_int(x), __float_as_int(x)));         // quad_perm [1,0,3,2]
    x = step(x, dpp_i<0x4E>(__float_as_int(x), __float_as_int(x)));         // quad_perm [2,3,0,1]
    x = step(x, dpp_i<0x141>(__float_as_int(x), __float_as_int(x)));        // row_half_mirror
    x = step(x, dpp_i<0x140>(__float_as_int(x), __float_as_int(x)));        // row_mirror
    x = step(x, dpp_i<0x142, 0xA>(__float_as_int(x), __float_as_int(x)));   // row_bcast:15
    x = step(x, dpp_i<0x143, 0xC>(__float_as_int(x), __float_as_int(x)));   // row_bcast:31
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ int wave_min_i(int x)
{
    x = min(x, dpp_i<0xB1>(x, x));
    x = min(x, dpp_i<0x4E>(x, x));
    x = min(x, dpp_i<0x141>(x, x));
    x = min(x, dpp_i<0x140>(x, x));
    x = min(x, dpp_i<0x142, 0xA>(x, x));
    x = min(x, dpp_i<0x143, 0xC>(x, x));
    return __builtin_amdgcn_readlane(x, 63);
}

}  // namespace mccnn
