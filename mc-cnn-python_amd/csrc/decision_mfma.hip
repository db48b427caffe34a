// Decision network of the "accurate" MC-CNN (Zbontar & LeCun 2016, sec. 3.2) on the gfx950 matrix cores.
//
//   s(h,w,d) = sigmoid(wf . relu(W_n ... relu(W_2 . relu(aL[h,w] + aR[h,w-d]) + b_2) ... + b_n) + bf)      w >= d
//   lcv[h,w,d] = -s,  rcv[h,w-d,d] = -s;  border columns: the fill kernels of cost_volume.hip, unchanged.
//
// aL = W1L.fL + b1 and aR = W1R.fR are the two halves of the first fully-connected layer, evaluated once per pixel by
// the caller (the layer is linear in the concatenation); the per-voxel work starts at relu(aL + aR).
//
// Layout: voxels on the lanes, hidden units in the accumulator registers.  A wave owns one pixel (h, w) and 32
// consecutive disparities; Y = W . X with A = weights (32 units x 16 k), B = activations (16 k x 32 voxels) gives the
// layer's result as twelve 32 x 32 tiles whose column (voxel) is the lane and whose rows (units) are the 16 registers:
// exactly what the next layer's B operand wants - registers 8s .. 8s+7 of tile t are the fragment of k-step 2t + s,
// no lane movement, no LDS.  The k order inside such a step is permuted (element j of lane half h is unit
// 16s + 8(j>>2) + 4h + (j&3) of the tile); mccnn_decision_pack lays the weights out to match.
//
// Registers per lane: 192 float32 activations (layer input) + 192 float32 accumulators (layer output); the f16
// fragments of a k-step are made from the activations when the step begins.  One wave per SIMD, four waves (four
// neighbouring pixels, the same 32 disparities) per workgroup.
//
// Weights: a 384 x 384 layer is 288 KiB as f16 and 576 KiB split - it stays in L2 and streams through LDS in 12 KiB
// chunks of twelve 1 KiB fragments (64 lanes x 8 f16 in the order the waves read them), double-buffered, one barrier
// per chunk, shared by the four waves.  Split: chunk c = (k-step c>>1, tiles 6(c&1) .. +5, hi and lo fragment of each);
// f16: chunk c = (k-step c, tiles 0 .. 11).
//
// Precisions (one template): SPLIT carries every float32 operand as two f16 numbers (x * scale = hi + lo, 22
// significand bits) and every multiply as three products hi*hi + hi*lo + lo*hi, float32 accumulation; the other form
// is one f16 product per multiply.  Activations carry the factor 256 and saturate at |x| * 256 = 65504, the contract
// of conv_mfma.hip: a clamped activation of a stored voxel raises the saturation flag.  So does a NaN in aL + aR or in
// a hidden layer's pre-activation (the tests are made before the ReLU, which would turn NaN into 0); -inf is what relu
// makes of it, 0, and raises nothing.
#include "common.h"

namespace mccnn {

constexpr int DK_UNITS = 384;
constexpr int DK_TILES = DK_UNITS / 32;
constexpr int DK_CHUNK = 12 * 1024;          // bytes: twelve fragments of 64 lanes x 16 B
constexpr float DK_ACT_SCALE = 256.f;
constexpr int DK_MAX_D = 1024;

using dk_f32x16 = __attribute__((ext_vector_type(16))) float;
typedef _Float16 dk_h8 __attribute__((ext_vector_type(8)));

template <bool SPLIT>
constexpr int dk_chunks() { return SPLIT ? 48 : 24; }   // per layer

// weights [n_layers][384 out][384 in] float32 -> fragments in consumption order (see above), scaled by `scale`
template <bool SPLIT>
__global__ __launch_bounds__(256) void decision_pack_kernel(const float *__restrict__ w, int n_layers, float scale,
                                                            dk_h8 *__restrict__ packed)
{
    constexpr int NC = dk_chunks<SPLIT>();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n_layers * NC * 12 * 64) return;
    const int lane = (int)(idx & 63), f = (int)((idx >> 6) % 12), c = (int)((idx / (64 * 12)) % NC);
    const int layer = (int)(idx / (64 * 12 * NC));
    const int s = SPLIT ? c >> 1 : c;
    const int t = SPLIT ? 6 * (c & 1) + (f >> 1) : f;
    const bool lo_part = SPLIT && (f & 1);
    const int r = lane & 31, h = lane >> 5;
    dk_h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
        const float x = __builtin_amdgcn_fmed3f(w[((size_t)layer * DK_UNITS + 32 * t + r) * DK_UNITS + k] * scale,
                                                -65504.f, 65504.f);
        const _Float16 hi = (_Float16)x;
        o[j] = lo_part ? (_Float16)(x - (float)hi) : hi;
    }
    packed[idx] = o;
}

// lcv / rcv element (pixel p, disparity d) at p * sp + d * sd: pixel-major sp = Dp, sd = 1; plane-major sp = 1, sd = H*W
template <bool SPLIT>
__global__ __launch_bounds__(256) void decision_kernel(const float *__restrict__ aL, const float *__restrict__ aR,
                                                       const uint4 *__restrict__ packed, const float *__restrict__ bias,
                                                       const float *__restrict__ wfin, float bfin, int n_layers,
                                                       float inv_scale, int H, int W, int D, float *__restrict__ lcv,
                                                       float *__restrict__ rcv, size_t sp, size_t sd,
                                                       int *__restrict__ sat_flag)
{
    constexpr int NC = dk_chunks<SPLIT>();
    __shared__ __attribute__((aligned(16))) char lds[2 * DK_CHUNK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int v = lane & 31, hh = lane >> 5;
    const int d0 = (int)blockIdx.z * 32;
    if ((int)blockIdx.x * 4 + 3 < d0) return;          // every voxel of the workgroup has w < d: border fill
    const int w = (int)blockIdx.x * 4 + wave, h = blockIdx.y, d = d0 + v;
    const bool valid = w < W && d < D && d <= w;
    const int wl = min(w, W - 1), xr = valid ? w - d : 0;
    const size_t rowbase = (size_t)h * W;
    const float *pl = aL + (rowbase + wl) * DK_UNITS + 4 * hh;
    const float *pr = aR + (rowbase + xr) * DK_UNITS + 4 * hh;

    dk_f32x16 act[DK_TILES], acc[DK_TILES];
    bool over = false;
#pragma unroll
    for (int t = 0; t < DK_TILES; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a = *reinterpret_cast<const float4 *>(pl + 32 * t + 8 * g);
            const float4 b = *reinterpret_cast<const float4 *>(pr + 32 * t + 8 * g);
            const float x[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // the range test on the pre-ReLU value: NaN fails it (fmaxf(NaN, 0) is 0), negative values pass
                over |= !(x[i] * DK_ACT_SCALE <= 65504.f);
                act[t][4 * g + i] = fmaxf(x[i], 0.f);
            }
        }

    // chunk 0 of the first layer
    const int total = n_layers * NC;
    const uint4 *gsrc = packed + tid;
    uint4 nx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) nx[i] = gsrc[i * 256];
#pragma unroll
    for (int i = 0; i < 3; ++i) *reinterpret_cast<uint4 *>(lds + (tid + i * 256) * 16) = nx[i];
    __syncthreads();

    int gc = 0;
#pragma unroll 1
    for (int layer = 0; layer < n_layers; ++layer) {
#pragma unroll
        for (int t = 0; t < DK_TILES; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        dk_h8 bh, bl;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            // the next chunk on its way (the last one of all re-reads itself: unconditional loads keep the waits exact).
            // Known limit: with 192 activations in the 256 VGPRs the scheduler sinks these loads to their
            // LDS stores behind the products, so their latency is exposed; pinning them here made the allocator spill.
            const size_t nxt = (size_t)min(gc + 1, total - 1) * (DK_CHUNK / 16);
#pragma unroll
            for (int i = 0; i < 3; ++i) nx[i] = gsrc[nxt + i * 256];
            const char *buf = lds + (c & 1) * DK_CHUNK + lane * 16;
            const int s = SPLIT ? c >> 1 : c;
            if (!SPLIT || (c & 1) == 0) {
                const int tp = s >> 1, r0 = 8 * (s & 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = __builtin_amdgcn_fmed3f(act[tp][r0 + j] * DK_ACT_SCALE, -65504.f, 65504.f);
                    const _Float16 hi = (_Float16)x;
                    bh[j] = hi;
                    if (SPLIT) bl[j] = (_Float16)(x - (float)hi);
                }
            }
            if (SPLIT) {
#pragma unroll
                for (int f = 0; f < 6; ++f) {
                    const int t = 6 * (c & 1) + f;
                    const dk_h8 a_hi = *reinterpret_cast<const dk_h8 *>(buf + (2 * f) * 1024);
                    const dk_h8 a_lo = *reinterpret_cast<const dk_h8 *>(buf + (2 * f + 1) * 1024);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, bh, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bl, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bh, acc[t], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int t = 0; t < DK_TILES; ++t) {
                    const dk_h8 a = *reinterpret_cast<const dk_h8 *>(buf + t * 1024);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bh, acc[t], 0, 0, 0);
                }
            }
            char *dst = lds + ((c + 1) & 1) * DK_CHUNK;
#pragma unroll
            for (int i = 0; i < 3; ++i) *reinterpret_cast<uint4 *>(dst + (tid + i * 256) * 16) = nx[i];
            __syncthreads();
            ++gc;
        }
        // bias + ReLU: the accumulators become the next layer's input (or the final product's)
        const float *pb = bias + (size_t)layer * DK_UNITS + 4 * hh;
        // the range test is made before the ReLU, as above.  The last hidden layer feeds the float32 product and has
        // no range: against +inf the test is x != x, NaN alone.  (x <= 255.875 is x * 256 <= 65504: a power of two.)
        const float limit = layer + 1 < n_layers ? 65504.f / DK_ACT_SCALE : __builtin_inff();
#pragma unroll
        for (int t = 0; t < DK_TILES; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b = *reinterpret_cast<const float4 *>(pb + 32 * t + 8 * g);
                const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x = acc[t][4 * g + i] * inv_scale + bb[i];
                    over |= !(x <= limit);
                    act[t][4 * g + i] = fmaxf(x, 0.f);
                }
            }
    }

    // final layer (float32): this lane's 192 units, sixteen at a time as a tree, then the other lane half's
    float z = 0.f;
#pragma unroll
    for (int t = 0; t < DK_TILES; ++t) {
        float p[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 q = *reinterpret_cast<const float4 *>(wfin + 4 * hh + 32 * t + 8 * g);
            p[4 * g + 0] = act[t][4 * g + 0] * q.x;
            p[4 * g + 1] = act[t][4 * g + 1] * q.y;
            p[4 * g + 2] = act[t][4 * g + 2] * q.z;
            p[4 * g + 3] = act[t][4 * g + 3] * q.w;
        }
#pragma unroll
        for (int n = 8; n >= 1; n >>= 1)
#pragma unroll
            for (int i = 0; i < n; ++i) p[i] = p[i] + p[i + n];
        z += p[0];
    }
    z = z + __shfl_xor(z, 32, 64);
    z += bfin;
    const float out = -(1.f / (1.f + expf(-z)));
    if (valid) {
        if (hh == 0)
            lcv[(rowbase + w) * sp + (size_t)d * sd] = out;
        else
            rcv[(rowbase + (w - d)) * sp + (size_t)d * sd] = out;
    }
    // a stored voxel's activation left the f16 range (x * 256 > 65504: clamped) or was NaN: the score is not the network's
    if (sat_flag && __builtin_amdgcn_ballot_w64(over && valid) != 0 && lane == 0) atomicOr(sat_flag, 1);
}

static bool dk_mode_ok(int mode) { return mode == MCCNN_CV_EXACT || mode == MCCNN_CV_MFMA; }
// finite, and scale * 256 and 1 / (scale * 256) normal float32 numbers (NaN fails either comparison): inf would pack
// w * inf and make the reciprocal zero
static bool dk_scale_ok(float scale) { return scale >= 0x1p-126f && scale <= 0x1p118f; }

static int decision_check(const char *who, const void *aL, const void *aR, const void *packed, const void *biases,
                          const void *w_final, const void *lcv, const void *rcv, int H, int W, int C, int units, int n_fc,
                          int D, int mode)
{
    MCCNN_REQUIRE(aL && aR && packed && biases && w_final && lcv && rcv, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0 && D > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(dk_mode_ok(mode), MCCNN_E_INVALID, "%s: unknown mode %d", who, mode);
    MCCNN_REQUIRE(C == 64 || C == 112, MCCNN_E_UNSUPPORTED, "%s: C=%d, the decision kernel serves 64 or 112 feature maps",
                  who, C);
    MCCNN_REQUIRE(units == DK_UNITS, MCCNN_E_UNSUPPORTED, "%s: %d units, the decision kernel is built for %d", who, units,
                  DK_UNITS);
    MCCNN_REQUIRE(n_fc == 3 || n_fc == 4, MCCNN_E_UNSUPPORTED,
                  "%s: %d fully-connected layers, the decision kernel serves 3 or 4", who, n_fc);
    MCCNN_REQUIRE(D >= 2 && D <= DK_MAX_D, MCCNN_E_UNSUPPORTED, "%s: D=%d outside [2, %d]", who, D, DK_MAX_D);
    MCCNN_REQUIRE(D <= W - 2, MCCNN_E_UNSUPPORTED,
                  "%s: D=%d needs W >= D+2 (the border recurrence is degenerate beyond that), W=%d", who, D, W);
    MCCNN_REQUIRE(H <= 65535 && cdiv(D, 32) <= 65535, MCCNN_E_UNSUPPORTED, "%s: H=%d exceeds the grid", who, H);
    return 0;
}

template <bool SPLIT>
static void decision_launch(const float *aL, const float *aR, const void *packed, const float *biases,
                            const float *w_final, float b_final, int n_layers, float weight_scale, int H, int W, int D,
                            float *lcv, float *rcv, size_t sp, size_t sd, int *sat, hipStream_t s)
{
    const dim3 grid(cdiv(W, 4), H, cdiv(D, 32));
    hipLaunchKernelGGL(decision_kernel<SPLIT>, grid, dim3(256), 0, s, aL, aR, reinterpret_cast<const uint4 *>(packed),
                       biases, w_final, b_final, n_layers, 1.f / (weight_scale * DK_ACT_SCALE), H, W, D, lcv, rcv, sp, sd,
                       sat);
}

}  // namespace mccnn

extern "C" size_t mccnn_decision_pack_bytes(int n_fc, int units, int mode)
{
    using namespace mccnn;
    if (units != DK_UNITS || (n_fc != 3 && n_fc != 4) || !dk_mode_ok(mode)) return 0;
    return (size_t)(n_fc - 1) * (mode == MCCNN_CV_EXACT ? dk_chunks<true>() : dk_chunks<false>()) * DK_CHUNK;
}

extern "C" int mccnn_decision_pack(const float *weights, int n_fc, int units, float weight_scale, int mode, void *packed,
                                   mccnn_stream_t stream)
{
    using namespace mccnn;
    MCCNN_REQUIRE(weights && packed, MCCNN_E_INVALID, "mccnn_decision_pack: null pointer");
    MCCNN_REQUIRE(dk_mode_ok(mode), MCCNN_E_INVALID, "mccnn_decision_pack: unknown mode %d", mode);
    MCCNN_REQUIRE(units == DK_UNITS, MCCNN_E_UNSUPPORTED, "mccnn_decision_pack: %d units, the decision kernel is built for %d",
                  units, DK_UNITS);
    MCCNN_REQUIRE(n_fc == 3 || n_fc == 4, MCCNN_E_UNSUPPORTED,
                  "mccnn_decision_pack: %d fully-connected layers, the decision kernel serves 3 or 4", n_fc);
    MCCNN_REQUIRE(dk_scale_ok(weight_scale), MCCNN_E_INVALID,
                  "mccnn_decision_pack: weight_scale must be finite, in [2^-126, 2^118]");
    const int nl = n_fc - 1;
    const long n = (long)nl * (mode == MCCNN_CV_EXACT ? dk_chunks<true>() : dk_chunks<false>()) * 12 * 64;
    hipStream_t s = (hipStream_t)stream;
    if (mode == MCCNN_CV_EXACT)
        hipLaunchKernelGGL(decision_pack_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, weights, nl, weight_scale,
                           reinterpret_cast<dk_h8 *>(packed));
    else
        hipLaunchKernelGGL(decision_pack_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, weights, nl, weight_scale,
                           reinterpret_cast<dk_h8 *>(packed));
    return check_launch("mccnn_decision_pack");
}

extern "C" int mccnn_cost_volume_accurate(const float *aL, const float *aR, int H, int W, int C, int units, int n_fc, int D,
                                          const void *packed, const float *biases, const float *w_final, float b_final,
                                          float weight_scale, float *lcv, float *rcv, int mode, int *saturation_flag,
                                          mccnn_stream_t stream)
{
    using namespace mccnn;
    int rc = decision_check("mccnn_cost_volume_accurate", aL, aR, packed, biases, w_final, lcv, rcv, H, W, C, units, n_fc, D,
                            mode);
    if (rc) return rc;
    MCCNN_REQUIRE(dk_scale_ok(weight_scale), MCCNN_E_INVALID,
                  "mccnn_cost_volume_accurate: weight_scale must be finite, in [2^-126, 2^118]");
    hipStream_t s = (hipStream_t)stream;
    const size_t plane = (size_t)H * W;
    if (mode == MCCNN_CV_EXACT)
        decision_launch<true>(aL, aR, packed, biases, w_final, b_final, n_fc - 1, weight_scale, H, W, D, lcv, rcv, 1, plane,
                              saturation_flag, s);
    else
        decision_launch<false>(aL, aR, packed, biases, w_final, b_final, n_fc - 1, weight_scale, H, W, D, lcv, rcv, 1, plane,
                               saturation_flag, s);
    rc = check_launch("mccnn_cost_volume_accurate");
    if (rc) return rc;
    return launch_cost_volume_fill(lcv, rcv, D, H, W, s, "mccnn_cost_volume_accurate(fill)");
}

extern "C" int mccnn_cost_volume_accurate_hwd(const float *aL, const float *aR, int H, int W, int C, int units, int n_fc,
                                              int D, const void *packed, const float *biases, const float *w_final,
                                              float b_final, float weight_scale, float *lcv_hwd, float *rcv_hwd, int mode,
                                              int *saturation_flag, mccnn_stream_t stream)
{
    using namespace mccnn;
    int rc = decision_check("mccnn_cost_volume_accurate_hwd", aL, aR, packed, biases, w_final, lcv_hwd, rcv_hwd, H, W, C,
                            units, n_fc, D, mode);
    if (rc) return rc;
    MCCNN_REQUIRE(dk_scale_ok(weight_scale), MCCNN_E_INVALID,
                  "mccnn_cost_volume_accurate_hwd: weight_scale must be finite, in [2^-126, 2^118]");
    const int Dp = mccnn_hwd_pitch(D);
    MCCNN_REQUIRE((size_t)W * Dp * 4 < ((size_t)1 << 31), MCCNN_E_UNSUPPORTED,
                  "mccnn_cost_volume_accurate_hwd: a %d x %d row exceeds a buffer descriptor's reach", W, D);
    hipStream_t s = (hipStream_t)stream;
    if (mode == MCCNN_CV_EXACT)
        decision_launch<true>(aL, aR, packed, biases, w_final, b_final, n_fc - 1, weight_scale, H, W, D, lcv_hwd, rcv_hwd,
                              (size_t)Dp, 1, saturation_flag, s);
    else
        decision_launch<false>(aL, aR, packed, biases, w_final, b_final, n_fc - 1, weight_scale, H, W, D, lcv_hwd, rcv_hwd,
                               (size_t)Dp, 1, saturation_flag, s);
    rc = check_launch("mccnn_cost_volume_accurate_hwd");
    if (rc) return rc;
    return launch_cost_volume_fill_hwd(lcv_hwd, rcv_hwd, D, Dp, H, W, s, "mccnn_cost_volume_accurate_hwd(fill)");
}
