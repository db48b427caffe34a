// Semi-dense maps (include/mccnn.h has the binding definitions): the selection by validity, left-right status and
// confidence thresholds - one streaming launch - and the speckle filter, which needs the 4-connected components of the
// map.  The components come from a union-find by label equivalence in four launches whose count and sizes depend on
// H and W alone: no read-back, no convergence test, nothing that waits for another workgroup.
//   1 seed      labels[p] = the start of p's horizontal run inside its wave's 64 pixels (ballot + leading-zero count,
//               as fill_rows_kernel of kitti.hip finds its nearest valid lane); a run that enters the wave from the
//               left hangs under the pixel before it.  Invalid pixels get kNone.  counts[p] = 0.
//   2 unite     the vertical links, with a returning atomicMin on roots.  A link whose two pixels are already joined
//               through their left neighbours is skipped: a constant map unites one column.
//   3 compress  labels[p] = root(p), and counts[root] += the length of each run of equal roots, combined across the
//               workgroup's four waves and its four steps before one atomic add goes out.
//   4 finish    sizes[p] = counts[labels[p]], out[p] = disp[p] or +inf.
// Labels only ever decrease, and a label is always a pixel of the same component at a lower or equal index.  Inside
// launches 2 and 3 a label read is an agent-scope relaxed load and may be stale: a stale parent is still an ancestor,
// and what decides a union is the value the atomic returns, never a load.  Integer minima and sums commute, so labels
// (after 3), counts and sizes are functions of the map alone.
#include "common.h"

namespace mccnn {
namespace semi {

constexpr unsigned kNone = 0xFFFFFFFFu;      // the label of an invalid pixel; H*W <= 2^31 - 1 keeps it free
constexpr uint64_t kMaxPixels = 0x7FFFFFFFull;
constexpr int kThreads = 256;
constexpr int kSteps = 4;                    // compress_count_kernel: 1024 consecutive pixels per workgroup

__device__ __forceinline__ bool valid(float v) { return v >= 0.0f && v < __builtin_huge_valf(); }

__device__ __forceinline__ bool linked(float a, float b, float max_diff)
{
    return valid(a) && valid(b) && fabsf(a - b) <= max_diff;
}

__device__ __forceinline__ unsigned ld(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void st(unsigned *p, unsigned v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The lowest label reachable from x by the loads this lane sees: the root, or (stale) an ancestor.
__device__ __forceinline__ unsigned find(const unsigned *L, unsigned x)
{
    for (;;) {
        const unsigned p = ld(L + x);
        if (p == x) return x;
        x = p;
    }
}

// Joins the sets of a and b.  Every round the larger of the two candidates strictly decreases, so the loop ends; it
// waits for nobody.  atomicMin returns what the word really held: the candidate was a root exactly when that is itself.
// Otherwise the word's old parent is handed on to the next round, whether the minimum replaced it or not.
__device__ __forceinline__ void unite(unsigned *L, unsigned a, unsigned b)
{
    for (;;) {
        a = find(L, a);
        b = find(L, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(kThreads) void seed_kernel(const float *__restrict__ disp, unsigned N, unsigned W,
                                                        float max_diff, unsigned *__restrict__ labels,
                                                        unsigned *__restrict__ counts)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = p < N;
    const float v = in ? disp[p] : -1.0f;
    const bool left = in && (p % W) != 0 && linked(v, disp[p - 1], max_diff);
    const unsigned long long starts = __ballot(!left) | 1ull;
    const int s = 63 - __builtin_clzll(starts & (~0ull >> (63 - lane)));    // the run's first lane in this wave
    if (!in) return;
    unsigned l = p - (unsigned)(lane - s);
    if (lane == 0 && left) l = p - 1;
    labels[p] = valid(v) ? l : kNone;
    counts[p] = 0;
}

__global__ __launch_bounds__(kThreads) void unite_kernel(const float *__restrict__ disp, unsigned N, unsigned W,
                                                         float max_diff, unsigned *labels)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (p >= N || p < W) return;
    const float a = disp[p], u = disp[p - W];
    if (!linked(a, u, max_diff)) return;
    if (p % W != 0) {
        const float al = disp[p - 1], ul = disp[p - W - 1];
        if (linked(a, al, max_diff) && linked(u, ul, max_diff) && linked(al, ul, max_diff)) return;
    }
    unite(labels, p, p - W);
}

// One workgroup takes kSteps * 256 consecutive pixels (row ends do not matter: equal roots are one component).  A run
// of equal roots that reaches the end of a step is carried into the next one in registers (the same value in every
// thread) and added once when it ends, so a map that is one component costs one add per 1024 pixels.
__global__ __launch_bounds__(kThreads) void compress_count_kernel(unsigned N, unsigned *labels, unsigned *counts)
{
    __shared__ unsigned s_root[kThreads];
    __shared__ unsigned long long s_heads[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)blockIdx.x * (kThreads * kSteps);
    unsigned carry_root = kNone, carry_cnt = 0;
    for (int it = 0; it < kSteps; ++it) {
        const size_t p = base + (size_t)it * kThreads + tid;
        unsigned r = kNone;
        if (p < N) {
            const unsigned l = ld(labels + p);
            if (l != kNone) {
                r = find(labels, l);
                if (r != l) st(labels + p, r);
            }
        }
        s_root[tid] = r;
        __syncthreads();
        const bool head = r != (tid ? s_root[tid - 1] : carry_root);
        const unsigned long long m = __ballot(head);
        if (lane == 0) s_heads[wv] = m;
        __syncthreads();
        unsigned long long h[kThreads / 64];
        int first = kThreads, last = -1;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            h[w] = s_heads[w];
            if (h[w]) {
                if (first == kThreads) first = w * 64 + __builtin_ctzll(h[w]);
                last = w * 64 + 63 - __builtin_clzll(h[w]);
            }
        }
        if (head && r != kNone) {                  // the run that starts here ends at the next head; the last one is carried
            int next = kThreads;
            const unsigned long long rest = lane == 63 ? 0ull : m & (~0ull << (lane + 1));
            if (rest) {
                next = wv * 64 + __builtin_ctzll(rest);
            } else {
#pragma unroll
                for (int w = kThreads / 64 - 1; w >= 0; --w)
                    if (w > wv && h[w]) next = w * 64 + __builtin_ctzll(h[w]);
            }
            if (next != kThreads) atomicAdd(counts + r, (unsigned)(next - tid));
        }
        if (first == kThreads) {
            carry_cnt += kThreads;
        } else {
            if (tid == 0 && carry_root != kNone) atomicAdd(counts + carry_root, carry_cnt + (unsigned)first);
            carry_root = s_root[last];
            carry_cnt = (unsigned)(kThreads - last);
        }
        __syncthreads();
    }
    if (tid == 0 && carry_root != kNone) atomicAdd(counts + carry_root, carry_cnt);
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const float *__restrict__ disp, unsigned N, unsigned min_size,
                                                          const unsigned *__restrict__ labels,
                                                          const unsigned *__restrict__ counts, float *__restrict__ out,
                                                          uint32_t *__restrict__ sizes)
{
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (p >= N) return;
    const unsigned l = labels[p];
    const unsigned n = l == kNone ? 0u : counts[l];
    if (sizes) sizes[p] = n;
    if (out) out[p] = n >= min_size ? disp[p] : __builtin_huge_valf();
}

struct MinConf {
    float t[4];
};

__global__ __launch_bounds__(kThreads) void select_kernel(const float *__restrict__ disp, const int32_t *__restrict__ status,
                                                          const float *__restrict__ planes, size_t N, unsigned plane_measures,
                                                          unsigned use, MinConf mc, float *__restrict__ out)
{
    const size_t n = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const float v = disp[n];
    bool keep = valid(v);
    if (status) keep = keep && status[n] == 0;
    size_t k = 0;       // plane b's place among the planes of plane_measures; `planes` is touched for used planes only
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (plane_measures >> b & 1u) {
            if (use >> b & 1u) keep = keep && planes[k * N + n] >= mc.t[b];
            ++k;
        }
    }
    out[n] = keep ? v : __builtin_huge_valf();
}

static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace semi
}  // namespace mccnn

extern "C" int mccnn_semi_dense_select(const float *disp, const int32_t *status, const float *planes, int H, int W,
                                       unsigned plane_measures, unsigned use, const float *min_conf, int require_match,
                                       float *out, mccnn_stream_t stream)
{
    using namespace mccnn;
    using namespace mccnn::semi;
    const char *who = "mccnn_semi_dense_select";
    MCCNN_REQUIRE(disp && out, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE((plane_measures & ~15u) == 0 && (use & ~15u) == 0, MCCNN_E_INVALID,
                  "%s: plane_measures=0x%x, use=0x%x: bits above 15", who, plane_measures, use);
    MCCNN_REQUIRE((use & ~plane_measures) == 0, MCCNN_E_INVALID, "%s: use=0x%x is not a subset of plane_measures=0x%x", who,
                  use, plane_measures);
    MCCNN_REQUIRE(!use || (planes && min_conf), MCCNN_E_INVALID, "%s: use=0x%x with a null planes or min_conf", who, use);
    MCCNN_REQUIRE(!require_match || status, MCCNN_E_INVALID, "%s: require_match with a null status", who);
    MinConf mc = {{0.f, 0.f, 0.f, 0.f}};
    for (int b = 0; b < 4; ++b) {
        if (!(use >> b & 1u)) continue;
        mc.t[b] = min_conf[b];
        MCCNN_REQUIRE(mc.t[b] == mc.t[b], MCCNN_E_INVALID, "%s: min_conf[%d] is NaN", who, b);
    }
    const size_t N = (size_t)H * W, plane = N * sizeof(float);
    MCCNN_REQUIRE(!overlaps(out, plane, disp, plane), MCCNN_E_INVALID, "%s: out overlaps disp", who);
    MCCNN_REQUIRE(!require_match || !overlaps(out, plane, status, plane), MCCNN_E_INVALID, "%s: out overlaps status", who);
    MCCNN_REQUIRE(!use || !overlaps(out, plane, planes, plane * (size_t)__builtin_popcount(plane_measures)), MCCNN_E_INVALID,
                  "%s: out overlaps planes", who);
    MCCNN_REQUIRE((N + kThreads - 1) / kThreads <= 0x7FFFFFFFull, MCCNN_E_UNSUPPORTED, "%s: %d x %d pixels exceed grid.x", who,
                  H, W);
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       disp, require_match ? status : nullptr, use ? planes : nullptr, N, plane_measures, use, mc, out);
    return check_launch(who);
}

extern "C" size_t mccnn_speckle_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0 || (uint64_t)H * (uint64_t)W > mccnn::semi::kMaxPixels) return 0;
    return (size_t)H * W * 2 * sizeof(uint32_t);     // labels[H*W], counts[H*W]
}

extern "C" int mccnn_speckle_filter(const float *disp, int H, int W, float max_diff, unsigned min_size, float *out,
                                    uint32_t *sizes, void *scratch, size_t scratch_bytes, mccnn_stream_t stream)
{
    using namespace mccnn;
    using namespace mccnn::semi;
    const char *who = "mccnn_speckle_filter";
    MCCNN_REQUIRE(disp && scratch, MCCNN_E_INVALID, "%s: null pointer", who);
    MCCNN_REQUIRE(out || sizes, MCCNN_E_INVALID, "%s: out and sizes are both null", who);
    MCCNN_REQUIRE(H > 0 && W > 0, MCCNN_E_INVALID, "%s: non-positive size", who);
    MCCNN_REQUIRE(max_diff >= 0.0f, MCCNN_E_INVALID, "%s: max_diff=%g, expected a value >= 0", who, (double)max_diff);
    MCCNN_REQUIRE(min_size >= 1, MCCNN_E_INVALID, "%s: min_size=0, expected at least 1", who);
    MCCNN_REQUIRE((uint64_t)H * (uint64_t)W <= kMaxPixels, MCCNN_E_UNSUPPORTED,
                  "%s: %d x %d pixels, a label holds H*W <= %llu", who, H, W, (unsigned long long)kMaxPixels);
    const size_t need = mccnn_speckle_scratch_bytes(H, W), plane = need / 2;
    MCCNN_REQUIRE(scratch_bytes >= need, MCCNN_E_SCRATCH, "%s: scratch of %zu bytes, mccnn_speckle_scratch_bytes(%d, %d) = %zu",
                  who, scratch_bytes, H, W, need);
    MCCNN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15u) == 0, MCCNN_E_SCRATCH, "%s: scratch must be 16-byte aligned", who);
    MCCNN_REQUIRE(!overlaps(out, plane, disp, plane) && !overlaps(sizes, plane, disp, plane), MCCNN_E_INVALID,
                  "%s: output overlaps disp", who);
    MCCNN_REQUIRE(!overlaps(out, plane, sizes, plane), MCCNN_E_INVALID, "%s: out overlaps sizes", who);
    MCCNN_REQUIRE(!overlaps(scratch, need, disp, plane) && !overlaps(scratch, need, out, plane) &&
                      !overlaps(scratch, need, sizes, plane),
                  MCCNN_E_INVALID, "%s: scratch overlaps a map", who);
    const unsigned N = (unsigned)((size_t)H * W);
    unsigned *labels = static_cast<unsigned *>(scratch), *counts = labels + N;
    hipStream_t s = (hipStream_t)stream;
    const dim3 per_pixel((N + kThreads - 1) / kThreads), block(kThreads);
    hipLaunchKernelGGL(seed_kernel, per_pixel, block, 0, s, disp, N, (unsigned)W, max_diff, labels, counts);
    hipLaunchKernelGGL(unite_kernel, per_pixel, block, 0, s, disp, N, (unsigned)W, max_diff, labels);
    hipLaunchKernelGGL(compress_count_kernel, dim3((N + kThreads * kSteps - 1) / (kThreads * kSteps)), block, 0, s, N, labels,
                       counts);
    hipLaunchKernelGGL(finish_kernel, per_pixel, block, 0, s, disp, N, min_size, labels, counts, out, sizes);
    return check_launch(who);
}
