/*
 * mccnn_oracle.c - CPU restatement of the reference's stereo-matching hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  This file is the parity checker for the HIP path: only tests/,
 * __graft_entry__.smoke() and bench.py's `cpu_baseline` leg may build, load or call it.  The product
 * (mc-cnn-python_amd/) never links or imports anything under oracle/ and fails loudly without its HIP library.
 *
 * Every function restates one reference function, loop for loop in the reference's own evaluation order so that
 * float32 results are bit-identical to the reference run under NumPy 2.x.  Pinned by the .npz files in tests/golden, which
 * were produced by executing /root/reference/src/process_functional.py itself: ref_*.npz (tests/golden/gen_golden.py,
 * whole pairs at the default settings, D <= 16; tests/test_oracle_golden.py) and route_*.npz
 * (tests/golden/gen_route_golden.py: D up to 1024, arms up to 31, all penalty classes, +-inf / -0.0, W = 255 .. 257;
 * tests/test_reference_routes_cpu.py), and by tests/test_oracle_vs_reference_cpu.py, which runs the reference beside
 * these functions wherever it is present.  One stated departure: a NaN cost in orc_sgm_pass (the reference's np.amin
 * propagates it to the whole line, the `<` chain here does not).
 * "pf:" abbreviates /root/reference/src/process_functional.py.
 *
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC (see oracle/Makefile).  -ffp-contract=off is
 * load-bearing: the reference never fuses a multiply with an add.
 *
 * Layouts: images [H,W] float32 (the reference's [H,W,1]); features [H,W,C]; volumes [D,H,W]; maps [H,W].
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define IDX3(d, h, w, H, W) (((size_t)(d) * (size_t)(H) + (size_t)(h)) * (size_t)(W) + (size_t)(w))

/* ---- NumPy float32 add.reduce over a contiguous run (numpy/_core/src/umath/loops_utils.h.src,
 * pairwise_sum): n < 8 plain loop; n <= 128 eight accumulators combined as a fixed tree, tail added
 * sequentially; larger n split recursively.  np.sum(...) then adds the result to the identity 0. ------------- */
static float np_pairwise_sum_f32(const float *a, long n, long stride)
{
    if (n < 8) {
        float res = 0.f;
        for (long i = 0; i < n; i++) res += a[i * stride];
        return res;
    } else if (n <= 128) {
        float r[8], res;
        long i;
        for (int j = 0; j < 8; j++) r[j] = a[j * stride];
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[(i + j) * stride];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i * stride];
        return res;
    } else {
        long n2 = n / 2;
        n2 -= n2 % 8;
        return np_pairwise_sum_f32(a, n2, stride) + np_pairwise_sum_f32(a + n2 * stride, n - n2, stride);
    }
}

static float np_sum_f32(const float *a, long n)
{
    return 0.f + np_pairwise_sum_f32(a, n, 1);
}

/* np.linalg.norm of a one-element float32 vector: sqrt(x.dot(x)) (pf:512,520,525,533,588,596,615,623)
 * and sqrt(add.reduce(x*x, axis=-1)) for the [h,w,1] patch (pf:459). */
static float norm1(float x)
{
    float sq = x * x;
    return sqrtf(sq);
}

/* =========================================================================================================
 * a2  compute_cost_volume (pf:78-113)
 * ========================================================================================================= */
void orc_cost_volume(const float *fl, const float *fr, int H, int W, int C, int D, float *lcv, float *rcv)
{
    /* The border fills below index columns d - 1 and W - d - 3 .. W - d: outside [0, W) once D > W - 2, where the
     * reference is degenerate too.  Such a call writes nothing (the Python wrapper refuses it before). */
    if (D < 1 || D > W - 2) return;
    float *prod = (float *)malloc(sizeof(float) * (size_t)C);
    memset(lcv, 0, sizeof(float) * (size_t)D * H * W); /* pf:82 np.zeros */
    memset(rcv, 0, sizeof(float) * (size_t)D * H * W); /* pf:102 */
    /* pf:87-91: left[d,:,d:] = sum(fl[:, d:] * fr[:, :W-d], axis=-1) */
    for (int d = 0; d < D && d < W; d++)
        for (int h = 0; h < H; h++)
            for (int w = d; w < W; w++) {
                const float *a = fl + ((size_t)h * W + w) * C;
                const float *b = fr + ((size_t)h * W + (w - d)) * C;
                for (int c = 0; c < C; c++) prod[c] = a[c] * b[c];
                lcv[IDX3(d, h, w, H, W)] = np_sum_f32(prod, C);
            }
    /* pf:94-95: for d = D-1..1: left[d:D, :, d-1] = mean(left[d:D, :, d:d+3], axis=-1) */
    for (int d = D - 1; d >= 1; d--) {
        int hi = d + 3 < W ? d + 3 : W; /* NumPy clips the slice end */
        int cnt = hi - d;
        for (int dd = d; dd < D; dd++)
            for (int h = 0; h < H; h++) {
                float s = 0.f;
                for (int w = d; w < hi; w++) s += lcv[IDX3(dd, h, w, H, W)];
                lcv[IDX3(dd, h, d - 1, H, W)] = s / (float)cnt;
            }
    }
    /* pf:103-104: right[d,:,:W-d] = left[d,:,d:] */
    for (int d = 0; d < D && d < W; d++)
        for (int h = 0; h < H; h++)
            for (int w = 0; w < W - d; w++) rcv[IDX3(d, h, w, H, W)] = lcv[IDX3(d, h, w + d, H, W)];
    /* pf:105-106: for d = D-1..1: right[d:D,:,W-d] = mean(right[d:D,:,W-d-3:W-d], axis=-1)
     * (requires W-d-3 >= 0, i.e. D <= W-2; the reference is degenerate beyond that) */
    for (int d = D - 1; d >= 1; d--) {
        int lo = W - d - 3;
        for (int dd = d; dd < D; dd++)
            for (int h = 0; h < H; h++) {
                float s = 0.f;
                for (int w = lo; w < W - d; w++) s += rcv[IDX3(dd, h, w, H, W)];
                rcv[IDX3(dd, h, W - d, H, W)] = s / 3.f;
            }
    }
    /* pf:111-112 */
    size_t n = (size_t)D * H * W;
    for (size_t i = 0; i < n; i++) {
        lcv[i] = -1.f * lcv[i];
        rcv[i] = -1.f * rcv[i];
    }
    free(prod);
}

/* =========================================================================================================
 * a3  compute_cross_region (pf:571-657)
 * arms[h,w,0..3] = number of pixels accepted upward, downward, leftward, rightward (self excluded).
 * ========================================================================================================= */
void orc_cross_arms(const float *img, int H, int W, float tau, int L, uint8_t *arms, int32_t *count)
{
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            float cur = img[(size_t)h * W + w];
            int up = 0, down = 0, left = 0, right = 0;
            int lim;
            /* pf:585-591 top arm: h_bias = 0 (self) .. min(L, h+1)-1, stop at the first failure */
            lim = L < h + 1 ? L : h + 1;
            for (int b = 0; b < lim; b++) {
                if (norm1(cur - img[(size_t)(h - b) * W + w]) >= tau) break;
                if (b > 0) up++;
            }
            /* pf:593-599 bottom arm: h_bias = 1 .. min(L, H-h)-1 */
            lim = L < H - h ? L : H - h;
            for (int b = 1; b < lim; b++) {
                if (norm1(cur - img[(size_t)(h + b) * W + w]) >= tau) break;
                down++;
            }
            /* pf:612-618 left arm */
            lim = L < w + 1 ? L : w + 1;
            for (int b = 0; b < lim; b++) {
                if (norm1(cur - img[(size_t)h * W + (w - b)]) >= tau) break;
                if (b > 0) left++;
            }
            /* pf:620-626 right arm */
            lim = L < W - w ? L : W - w;
            for (int b = 1; b < lim; b++) {
                if (norm1(cur - img[(size_t)h * W + (w + b)]) >= tau) break;
                right++;
            }
            uint8_t *a = arms + ((size_t)h * W + w) * 4;
            a[0] = (uint8_t)up;
            a[1] = (uint8_t)down;
            a[2] = (uint8_t)left;
            a[3] = (uint8_t)right;
        }
    /* pf:640-653 union_region_num = sum over the vertical arm of the horizontal arm sizes */
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            const uint8_t *a = arms + ((size_t)h * W + w) * 4;
            int n = 0;
            for (int q = h - a[0]; q <= h + a[1]; q++) {
                const uint8_t *aq = arms + ((size_t)q * W + w) * 4;
                n += aq[2] + aq[3] + 1;
            }
            count[(size_t)h * W + w] = n;
        }
}

/* Explicit coordinate list in the reference's order (pf:637-655): vertical arm (self, up.., down..) x
 * horizontal arm of each of those pixels (self, left.., right..); padded with (-1,-1). region: [H,W,maxn,2]. */
void orc_cross_region(const float *img, int H, int W, float tau, int L, int32_t *region, int32_t *num)
{
    uint8_t *arms = (uint8_t *)malloc((size_t)H * W * 4);
    int maxn = (2 * L) * (2 * L);
    orc_cross_arms(img, H, W, tau, L, arms, num);
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            const uint8_t *a = arms + ((size_t)h * W + w) * 4;
            int32_t *r = region + ((size_t)h * W + w) * maxn * 2;
            int n = 0;
            int nv = 1 + a[0] + a[1];
            for (int v = 0; v < nv; v++) {
                int q = v == 0 ? h : (v <= a[0] ? h - v : h + (v - a[0]));
                const uint8_t *aq = arms + ((size_t)q * W + w) * 4;
                int nh = 1 + aq[2] + aq[3];
                for (int z = 0; z < nh; z++) {
                    int x = z == 0 ? w : (z <= aq[2] ? w - z : w + (z - aq[2]));
                    r[2 * n] = q;
                    r[2 * n + 1] = x;
                    n++;
                }
            }
            for (int i = n; i < maxn; i++) {
                r[2 * i] = -1;
                r[2 * i + 1] = -1;
            }
        }
    free(arms);
}

/* =========================================================================================================
 * a4  cost_volume_aggregation, one volume (pf:149-163 / 166-180): `iters` rounds of the flat float32
 * running sum over the cross region in list order, divided by the region size.  vol is overwritten.
 * ========================================================================================================= */
void orc_cbca(const float *img, float *vol, int D, int H, int W, float tau, int L, int iters)
{
    uint8_t *arms = (uint8_t *)malloc((size_t)H * W * 4);
    int32_t *cnt = (int32_t *)malloc(sizeof(int32_t) * (size_t)H * W);
    float *tmp = (float *)malloc(sizeof(float) * (size_t)D * H * W);
    float *src = vol, *dst = tmp;
    orc_cross_arms(img, H, W, tau, L, arms, cnt);
    for (int it = 0; it < iters; it++) {
        for (int d = 0; d < D; d++) {
            const float *pl = src + (size_t)d * H * W;
            float *po = dst + (size_t)d * H * W;
            for (int h = 0; h < H; h++)
                for (int w = 0; w < W; w++) {
                    const uint8_t *a = arms + ((size_t)h * W + w) * 4;
                    float s = 0.f; /* pf:157 */
                    int nv = 1 + a[0] + a[1];
                    for (int v = 0; v < nv; v++) {
                        int q = v == 0 ? h : (v <= a[0] ? h - v : h + (v - a[0]));
                        const uint8_t *aq = arms + ((size_t)q * W + w) * 4;
                        const float *row = pl + (size_t)q * W;
                        s += row[w];
                        for (int z = 1; z <= aq[2]; z++) s += row[w - z];
                        for (int z = 1; z <= aq[3]; z++) s += row[w + z];
                    }
                    po[(size_t)h * W + w] = s / (float)cnt[(size_t)h * W + w]; /* pf:161 */
                }
        }
        float *t = src;
        src = dst;
        dst = t;
    }
    if (src != vol) memcpy(vol, src, sizeof(float) * (size_t)D * H * W);
    free(arms);
    free(cnt);
    free(tmp);
}

/* =========================================================================================================
 * a6  semi_global_matching (pf:476-568): one axis-aligned direction, in place.
 * side: 0 = "L" (penalties from the right image at w-d), 1 = "R" (left image at w+d).
 * p1, p2, q1, q2, thr arrive as the float32 roundings NumPy applies to the Python scalars.
 * ========================================================================================================= */
static inline float pymin(float a, float b) { return b < a ? b : a; } /* Python min(): first wins ties */

void orc_sgm_pass(const float *img_l, const float *img_r, float *vol, int D, int H, int W, int rh, int rw,
                  float p1, float p2, float q1, float q2, float thr, int side)
{
    int starth, endh, steph, startw, endw, stepw;
    if (rh >= 0) { starth = rh; endh = H; steph = 1; } else { starth = H + rh - 1; endh = -1; steph = -1; }
    if (rw >= 0) { startw = rw; endw = W; stepw = 1; } else { startw = W + rw - 1; endw = -1; stepw = -1; }
    const float *self = side == 0 ? img_l : img_r;
    const float *other = side == 0 ? img_r : img_l;
    float *P1 = (float *)malloc(sizeof(float) * (size_t)D);
    float *P2 = (float *)malloc(sizeof(float) * (size_t)D);
    float *nw = (float *)malloc(sizeof(float) * (size_t)D);
    const float p1q1 = p1 / q1, p1q2 = p1 / q2, p2q1 = p2 / q1, p2q2 = p2 / q2; /* pf:538-541 */
    for (int h = starth; h != endh; h += steph)
        for (int w = startw; w != endw; w += stepw) {
            int hp = h - rh, wp = w - rw;
            float d1 = norm1(self[(size_t)h * W + w] - self[(size_t)hp * W + wp]); /* pf:512 / 525 */
            for (int d = 0; d < D; d++) {
                float d2 = 0.f; /* pf:507 zeros where skipped */
                if (side == 0) {
                    if (!(w - d < 0 || w - rw - d < 0)) /* pf:517-520 */
                        d2 = norm1(other[(size_t)h * W + (w - d)] - other[(size_t)hp * W + (w - rw - d)]);
                } else {
                    if (!(w + d >= W || w - rw + d >= W)) /* pf:530-533 */
                        d2 = norm1(other[(size_t)h * W + (w + d)] - other[(size_t)hp * W + (w - rw + d)]);
                }
                int c1 = (d1 < thr) && (d2 < thr);   /* pf:535 */
                int c2 = (d1 >= thr) && (d2 >= thr); /* pf:536 */
                if (c2) { P1[d] = p1q2; P2[d] = p2q2; }
                else if (!c1) { P1[d] = p1q1; P2[d] = p2q1; } /* pf:537 condition3 */
                else { P1[d] = p1; P2[d] = p2; }
            }
            /* pf:545-566 */
            float m = vol[IDX3(0, hp, wp, H, W)];
            for (int d = 1; d < D; d++) { /* np.amin */
                float v = vol[IDX3(d, hp, wp, H, W)];
                if (v < m) m = v;
            }
            for (int d = 0; d < D; d++) {
                float item1 = vol[IDX3(d, hp, wp, H, W)];
                float item4 = m + P2[d];
                float best;
                if (d == 0) {
                    float item3 = vol[IDX3(d + 1, hp, wp, H, W)] + P1[d];
                    best = pymin(item1, pymin(item3, item4)); /* pf:552 */
                } else if (d == D - 1) {
                    float item2 = vol[IDX3(d - 1, hp, wp, H, W)] + P1[d];
                    best = pymin(pymin(item1, item2), item4); /* pf:566 */
                } else {
                    float item2 = vol[IDX3(d - 1, hp, wp, H, W)] + P1[d];
                    float item3 = vol[IDX3(d + 1, hp, wp, H, W)] + P1[d];
                    best = pymin(pymin(item1, item2), pymin(item3, item4)); /* pf:559 */
                }
                float t = vol[IDX3(d, h, w, H, W)] + best;
                nw[d] = t - m;
            }
            for (int d = 0; d < D; d++) vol[IDX3(d, h, w, H, W)] = nw[d];
        }
    free(P1);
    free(P2);
    free(nw);
}

/* a5  SGM_average (pf:187-235), one side: four passes composed in place (the reference aliases one array,
 * pf:544,568) and the literal "(a+b+c+d)/4." of four aliases (pf:210,232).
 * p1v is float32(sgm_P1 / sgm_V) computed by the caller in double like Python does (pf:204). */
void orc_sgm_average(const float *img_l, const float *img_r, float *vol, int D, int H, int W, float p1, float p1v,
                     float p2, float q1, float q2, float thr, int side)
{
    orc_sgm_pass(img_l, img_r, vol, D, H, W, 0, 1, p1, p2, q1, q2, thr, side);
    orc_sgm_pass(img_l, img_r, vol, D, H, W, 0, -1, p1, p2, q1, q2, thr, side);
    orc_sgm_pass(img_l, img_r, vol, D, H, W, -1, 0, p1v, p2, q1, q2, thr, side);
    orc_sgm_pass(img_l, img_r, vol, D, H, W, 1, 0, p1v, p2, q1, q2, thr, side);
    size_t n = (size_t)D * H * W;
    for (size_t i = 0; i < n; i++) {
        float x = vol[i];
        float s = x + x;
        s = s + x;
        s = s + x;
        vol[i] = s / 4.f;
    }
}

/* =========================================================================================================
 * a7  disparity_prediction (pf:239-272), one volume: first strict minimum over d.
 * ========================================================================================================= */
void orc_wta(const float *vol, int D, int H, int W, float *disp)
{
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            float best = INFINITY;
            int bd = -1;
            for (int d = 0; d < D; d++) {
                float v = vol[IDX3(d, h, w, H, W)];
                if (v < best) { best = v; bd = d; }
            }
            disp[(size_t)h * W + w] = (float)bd;
        }
}

/* =========================================================================================================
 * a8  interpolation (pf:279-378)
 * ========================================================================================================= */
void orc_lr_status(const float *dl, const float *dr, int H, int W, int D, int32_t *status)
{
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            float lf = dl[(size_t)h * W + w];
            /* a disparity <= -1 (mccnn_wta's -1) or NaN indexes the right map out of bounds in the reference:
             * include/mccnn.h makes it an occlusion; (-1, 0) truncates to 0 (pf:287) */
            if (!(lf > -1.f)) { status[(size_t)h * W + w] = 2; continue; }
            int ld = (int)lf; /* pf:287 */
            int32_t st = 0;
            if (w < ld) { status[(size_t)h * W + w] = 2; continue; } /* pf:289-291 */
            float rd = dr[(size_t)h * W + (w - ld)];
            if (fabsf((float)ld - rd) <= 1.f) { status[(size_t)h * W + w] = 0; continue; } /* pf:294 */
            int lim = w + 1 < D ? w + 1 : D;
            for (int d = 0; d < lim; d++)
                if (fabsf((float)d - dr[(size_t)h * W + (w - d)]) <= 1.f) { st = 1; break; } /* pf:299-303 */
            if (st == 0) st = 2; /* pf:306-307 */
            status[(size_t)h * W + w] = st;
        }
}

static float median_small(float *v, int n)
{
    for (int i = 1; i < n; i++) { /* insertion sort, n <= 4 */
        float x = v[i];
        int j = i - 1;
        while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; j--; }
        v[j + 1] = x;
    }
    /* np.median -> np.mean of the middle value(s), float32; the mean's sum starts from +0, so -0.0 becomes +0.0 */
    if (n & 1) return 0.f + v[n / 2];
    return (0.f + (v[n / 2 - 1] + v[n / 2])) / 2.f;
}

void orc_interpolation(const float *dl, const float *dr, int H, int W, int D, float *out)
{
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)H * W);
    orc_lr_status(dl, dr, H, W, D, st);
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            size_t p = (size_t)h * W + w;
            if (st[p] == 0) { out[p] = dl[p]; continue; }
            if (st[p] == 1) { /* pf:316-356 */
                float nb[4];
                int c = 0;
                for (int x = w + 1; x < W; x++) if (st[(size_t)h * W + x] == 0) { nb[c++] = dl[(size_t)h * W + x]; break; }
                for (int x = w - 1; x >= 0; x--) if (st[(size_t)h * W + x] == 0) { nb[c++] = dl[(size_t)h * W + x]; break; }
                for (int y = h + 1; y < H; y++) if (st[(size_t)y * W + w] == 0) { nb[c++] = dl[(size_t)y * W + w]; break; }
                for (int y = h - 1; y >= 0; y--) if (st[(size_t)y * W + w] == 0) { nb[c++] = dl[(size_t)y * W + w]; break; }
                out[p] = c == 0 ? dl[p] : median_small(nb, c);
            } else { /* pf:358-373 occlusion: nearest match to the right */
                float v = dl[p];
                for (int x = w + 1; x < W; x++) if (st[(size_t)h * W + x] == 0) { v = dl[(size_t)h * W + x]; break; }
                out[p] = v;
            }
        }
    free(st);
}

/* =========================================================================================================
 * a9  subpixel_enhance (pf:381-400); float32 arithmetic as NumPy 2 evaluates it.
 * ========================================================================================================= */
void orc_subpixel(const float *dl, const float *vol, int D, int H, int W, float *out)
{
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            size_t p = (size_t)h * W + w;
            float d = dl[p];
            int im = (int)(d - 1.f), ip = (int)(d + 1.f), ic = (int)d;
            if (im < 0 || ip >= D) { out[p] = d; continue; } /* pf:390-391 */
            float cm = vol[IDX3(im, h, w, H, W)];
            float cp = vol[IDX3(ip, h, w, H, W)];
            float c = vol[IDX3(ic, h, w, H, W)];
            float num = cp - cm;
            float den = cp - 2.f * c;
            den = den + cm;
            den = 2.f * den;
            out[p] = d - num / den; /* pf:396 */
        }
}

/* =========================================================================================================
 * a10 median_filter (pf:403-421): clipped window, np.median.
 * ========================================================================================================= */
static int cmp_float(const void *a, const void *b)
{
    float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

void orc_median(const float *dl, int H, int W, int fh, int fw, float *out)
{
    int rh_ = (fh - 1) / 2, rw_ = (fw - 1) / 2;
    float *buf = (float *)malloc(sizeof(float) * (size_t)fh * fw);
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            int hs = h - rh_ > 0 ? h - rh_ : 0, he = h + rh_ + 1 < H ? h + rh_ + 1 : H;
            int ws = w - rw_ > 0 ? w - rw_ : 0, we = w + rw_ + 1 < W ? w + rw_ + 1 : W;
            int n = 0, has_nan = 0;
            for (int y = hs; y < he; y++)
                for (int x = ws; x < we; x++) {
                    float v = dl[(size_t)y * W + x];
                    if (v != v) has_nan = 1;
                    buf[n++] = v;
                }
            if (has_nan) { out[(size_t)h * W + w] = NAN; continue; } /* np.median propagates NaN */
            qsort(buf, n, sizeof(float), cmp_float);
            /* np.mean of the middle value(s): the float32 sum starts from +0 (a median of -0.0 is +0.0) */
            out[(size_t)h * W + w] = (n & 1) ? 0.f + buf[n / 2] : (0.f + (buf[n / 2 - 1] + buf[n / 2])) / 2.f;
        }
    free(buf);
}

/* =========================================================================================================
 * a11 bilateral_filter (pf:424-470).  `table` is the [fh,fw] float32 spatial kernel, which the reference
 * evaluates in float64 with util.normal and stores as float32 (pf:433-436, util.py:45-48); the caller
 * builds it the same way in Python so exp() is literally NumPy's.
 * ========================================================================================================= */
void orc_bilateral(const float *img, const float *dl, int H, int W, int fh, int fw, const float *table,
                   float thr, float *out)
{
    int ch = (fh - 1) / 2, cw = (fw - 1) / 2;
    float *wgt = (float *)malloc(sizeof(float) * (size_t)fh * fw);
    float *val = (float *)malloc(sizeof(float) * (size_t)fh * fw);
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            int hs = h - ch > 0 ? h - ch : 0, he = h + ch + 1 < H ? h + ch + 1 : H;
            int ws = w - cw > 0 ? w - cw : 0, we = w + cw + 1 < W ? w + cw + 1 : W;
            float cur = img[(size_t)h * W + w];
            int n = 0;
            for (int y = hs; y < he; y++)
                for (int x = ws; x < we; x++) {
                    float diff = norm1(img[(size_t)y * W + x] - cur);         /* pf:458-459 */
                    float gate = diff < thr ? 1.f : 0.f;                       /* pf:460 */
                    float f = gate * table[(ch + (y - h)) * fw + (cw + (x - w))]; /* pf:462 */
                    wgt[n] = f;
                    val[n] = f * dl[(size_t)y * W + x];                        /* pf:465 */
                    n++;
                }
            float wsum = np_sum_f32(wgt, n); /* pf:463 */
            float vsum = np_sum_f32(val, n); /* pf:466 */
            out[(size_t)h * W + w] = vsum / wsum;
        }
    free(wgt);
    free(val);
}

/* =========================================================================================================
 * a1  NET.features (model.py:51-64) on the once-zero-padded image (pf:20-25): VALID 3x3 cross-correlation,
 * HWIO weights, ReLU after all but the last layer, then x * rsqrt(max(sum x^2, 1e-12)).  float64 accumulate
 * ("fp64 restatement": the TensorFlow kernel's own summation order is not pinnable).
 * in: [Hin,Win,Cin] -> out: [Hin-2,Win-2,Cout]
 * ========================================================================================================= */
void orc_conv3x3_valid(const float *in, int Hin, int Win, int Cin, const float *w_hwio, const float *bias, int Cout,
                       int relu, float *out)
{
    int Ho = Hin - 2, Wo = Win - 2;
    double *acc = (double *)malloc(sizeof(double) * (size_t)Cout);
    for (int y = 0; y < Ho; y++)
        for (int x = 0; x < Wo; x++) {
            for (int o = 0; o < Cout; o++) acc[o] = 0.0;
            for (int ky = 0; ky < 3; ky++)
                for (int kx = 0; kx < 3; kx++) {
                    const float *px = in + ((size_t)(y + ky) * Win + (x + kx)) * Cin;
                    const float *wk = w_hwio + (size_t)(ky * 3 + kx) * Cin * Cout;
                    for (int c = 0; c < Cin; c++) {
                        double v = px[c];
                        const float *wr = wk + (size_t)c * Cout;
                        for (int o = 0; o < Cout; o++) acc[o] += v * (double)wr[o];
                    }
                }
            float *po = out + ((size_t)y * Wo + x) * Cout;
            for (int o = 0; o < Cout; o++) {
                double v = acc[o] + (double)bias[o];
                if (relu && v < 0.0) v = 0.0;
                po[o] = (float)v;
            }
        }
    free(acc);
}

void orc_l2_normalize(float *x, long npix, int C)
{
    for (long p = 0; p < npix; p++) {
        float *v = x + (size_t)p * C;
        double s = 0.0;
        for (int c = 0; c < C; c++) s += (double)v[c] * (double)v[c];
        if (s < 1e-12) s = 1e-12; /* tf.nn.l2_normalize epsilon (model.py:64) */
        double r = 1.0 / sqrt(s);
        for (int c = 0; c < C; c++) v[c] = (float)((double)v[c] * r);
    }
}
