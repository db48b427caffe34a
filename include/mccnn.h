/*
 * mccnn.h - C ABI of libmccnn_hip.so: the MI355X (gfx950) stereo-matching hot path.
 *
 * The reference (Jackie-Chou/MC-CNN-python) has no FFI layer: its hot path is eleven NumPy functions in
 * src/process_functional.py called by src/match.py:132-175.  Each entry point below replaces the interpreted
 * loop nest of one of those functions; the host-side mirror in mc-cnn-python_amd/src/process_functional.py keeps
 * the reference's Python signatures and calls these through ctypes (see INTEGRATION.md for the binding).
 * "pf:" = /root/reference/src/process_functional.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) owned by the caller; nothing is retained after return
 *   - no allocation, no synchronisation: work is enqueued on `stream` (a hipStream_t passed as void*);
 *     scratch, where needed, is passed in and sized by the matching *_scratch_bytes() query
 *   - return 0 on success, otherwise a negative MCCNN_E_* code or the positive hipError_t of the failed launch;
 *     mccnn_last_error_string() describes the last failure on the calling thread
 *   - float32 everywhere (the reference's dtype); sizes are ints, byte offsets are 64-bit inside
 *   - ONE piece of host-side state, the exception to "nothing is retained": mccnn_cross_arms / mccnn_cross_arms_pair
 *     remember, per support-buffer ADDRESS, the (H, W, L) they built it for (a mutex-guarded process-global map of at
 *     most 4096 entries, cleared when full).  The aggregation entry points consult it only to REFUSE a plane built for
 *     another image size or with longer arms than the L they are told (MCCNN_E_INVALID); addresses it has never seen
 *     pass.  It is keyed by address, not by allocation: a buffer that is freed and whose address is reused keeps its
 *     stale entry until the next mccnn_cross_arms on that address - which every correct use performs before
 *     aggregating with it.  No device memory is referenced by it.
 *
 * HBM layouts
 *   image     [H][W]        float32 (the reference's [H,W,1])
 *   features  [H][W][C]     float32, C = 64 (NET.features, NHWC)
 *   volume    "DHW" [D][H][W]   - the reference's layout; cost volume, the streaming CBCA and its WTA / sub-pixel
 *             "HWD" [H][W][Dp]  - pixel-major, Dp = mccnn_hwd_pitch(D); the SGM scanline kernels, and the whole
 *                                 bit-exact variant from the first aggregation on (mccnn_cbca_iter_hwd, mccnn_wta_hwd,
 *                                 mccnn_subpixel_hwd)
 *   support   mccnn_support_bytes(H,W) bytes: plane 0 [H][W] uint32 words (four 5-bit cross-arm lengths + 12-bit
 *             region size, mccnn_support_t), then four derived planes private to the aggregation kernels
 *   maps      [H][W]        float32 disparity maps, int32 status / region counts
 *
 * Memory contract (tests/test_memory_contract_gpu.py pins every sentence; "families" below note where one differs)
 *   Alignment.  On the pixel-major path - mccnn_cross_arms(_pair), mccnn_cost_volume_hwd (MCCNN_CV_EXACT),
 *     mccnn_cost_volume_vertical_hwd, mccnn_cost_volume_fill, mccnn_cbca_iter_hwd*, mccnn_cbca_iter_hwd_long*,
 *     mccnn_cbca_iter_prog*, the mccnn_sgm_* entry points, mccnn_wta_hwd, mccnn_subpixel_hwd, mccnn_dhw_to_hwd and
 *     mccnn_hwd_to_dhw - volumes, images, feature tensors and maps need only the alignment of their element, 4 bytes:
 *     the kernels reach them through vector loads and stores of 4 to 16 bytes per lane, which the hardware serves at
 *     any 4-byte-aligned address (the layout changes pick their 16-byte transposes only between two 16-byte-aligned
 *     bases).  A caller may carve all of those out of one arena.  The other entry points (plane-major aggregation,
 *     matrix-core cost volume, features, post-processing) have only ever been run on 16-byte-aligned pointers: keep
 *     theirs so.  Buffers whose layout is
 *     PRIVATE to the library must start on a 16-byte boundary: the support buffer (mccnn_support_bytes), the program
 *     buffers (mccnn_cbca_prog_bytes) and the SGM flag / scratch buffer (mccnn_sgm_scratch_bytes) - their planes are laid
 *     out in 16-byte steps from the base and read by scalar and packed loads.  A pointer that is not is refused on the
 *     host before anything is launched: MCCNN_E_INVALID for support and program buffers, MCCNN_E_SCRATCH for the SGM
 *     buffer (as mccnn_speckle_filter answers for its scratch).  The evaluation, ingest, KITTI and semi-dense entry
 *     points state the alignment of their own scratch and result buffers where they are declared.
 *   Pads.  A pixel-major volume has Dp - D pad entries per pixel (D % 4 != 0).  The pad entries of an INPUT never
 *     influence an entry d < D of any output, whatever they hold (stale costs, +-inf, NaN): every minimum, sum and
 *     neighbour lookup across d is masked to d < D.  The pad entries of an OUTPUT are left untouched by
 *     mccnn_cost_volume_hwd, mccnn_cost_volume_vertical_hwd and mccnn_cost_volume_fill(pixel_major != 0); after every
 *     other call that writes a pixel-major volume (the aggregation families, the SGM passes, mccnn_sgm_first_pass,
 *     mccnn_dhw_to_hwd, ...) they are unspecified.
 *   Bounds.  No call writes a byte outside the buffers documented for it, and no call reads one in a way that changes a
 *     result.  (Some kernels do read a few elements past a row or a plane inside the SAME buffer - a prefetch that is
 *     never used - and steer lanes without work to an offset their buffer descriptor drops.)  Buffers sized by a query
 *     (mccnn_support_bytes, mccnn_cbca_prog_bytes, mccnn_sgm_scratch_bytes) need exactly that many bytes.
 */
#ifndef MCCNN_H
#define MCCNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mccnn_stream_t; /* hipStream_t */

#define MCCNN_ABI_VERSION 7 /* 2: window-mask plane, *_hwd entry points; 3: saturation flags; 4: program-driven CBCA; 5: skip programs; 6: one-volume launches; 7: refresh launches, SGM flag planes as a call of their own; still 7 with the mccnn_ingest_* and the mccnn_decision_* / mccnn_cost_volume_accurate* entry points and mccnn_sample_patches, and with mccnn_evaluate, and with the mccnn_kitti_* entry points and mccnn_evaluate_kitti, and with mccnn_confidence / mccnn_confidence_hwd: purely additive, nothing that existed changed; still 7 with the memory contract below: no signature changed, and the only new refusals are support, program and SGM flag / scratch buffers that do not start on a 16-byte boundary (no allocator hands such a buffer out) */

#define MCCNN_E_INVALID (-1)     /* bad argument (null pointer, non-positive size, unsupported shape) */
#define MCCNN_E_UNSUPPORTED (-2) /* shape outside what the kernels were built for (e.g. D > 1024 for SGM) */
#define MCCNN_E_SCRATCH (-3)     /* scratch buffer too small */

#define MCCNN_SIDE_LEFT 0  /* the reference's choice == "L" */
#define MCCNN_SIDE_RIGHT 1 /* choice == "R" */

int mccnn_version(void);
const char *mccnn_last_error_string(void);

/* ---- a2  compute_cost_volume (pf:78-113) ------------------------------------------------------------------
 * lcv[d,h,w] = -<fl[h,w,:], fr[h,w-d,:]> for w >= d, border columns filled by the reference's 3-tap mean
 * recurrences, rcv[d,h,w] = lcv[d,h,w+d] (+ its own border recurrence).  Requires 1 <= D <= W-2.
 * mode MCCNN_CV_EXACT reproduces NumPy's pairwise float32 summation order bit for bit (C must be 64);
 * mode MCCNN_CV_MFMA contracts the 64 channels on the matrix cores (every float32 operand as two f16 numbers, three
 * v_mfma_f32_32x32x16_f16 products per K step, float32 accumulation): within 2e-6 of the float64 dot product, and of
 * MCCNN_CV_EXACT, on unit-norm features - the features must be unit vectors (|x| <= 1), as NET produces them; within
 * 8 x the error of NumPy's float32 pairwise sum + 2^-24 (measured: <= 3.6e-7, profiles/parity_cost_volume_mfma.json).
 * Non-finite and large features in MCCNN_CV_MFMA: a NaN feature propagates - every score of its pixel, and every border
 * entry filled from such a score, is NaN, the same set of entries as in MCCNN_CV_EXACT.  A finite feature with
 * |x * 1024| > 65504 is clamped to +-65504 / 1024 (its scores are finite and wrong).  +-inf is outside the contract. */
#define MCCNN_CV_EXACT 0
#define MCCNN_CV_MFMA 1
int mccnn_cost_volume(const float *fl, const float *fr, int H, int W, int C, int D, float *lcv, float *rcv, int mode,
                      mccnn_stream_t stream);

/* The same volumes written pixel-major ("HWD" [H][W][Dp], the layout the bit-exact variant keeps from here to WTA),
 * bit-identical to mccnn_cost_volume(mode) followed by mccnn_dhw_to_hwd for d < D (the Dp - D pad entries of a pixel
 * are not written), for MCCNN_CV_EXACT and (ABI 5) MCCNN_CV_MFMA alike; D <= 1024. */
int mccnn_cost_volume_hwd(const float *fl, const float *fr, int H, int W, int C, int D, float *lcv_hwd, float *rcv_hwd,
                          int mode, mccnn_stream_t stream);

/* The pixel-major MCCNN_CV_EXACT volumes with a VERTICAL SEARCH of +-vertical_range rows, for pairs whose rectification
 * leaves a residual vertical disparity (not in the reference).  fl, fr: [H][W][64] float32; r = vertical_range, 0 <= r <= 4.
 *   P(k; d,h,w) = the float32 score of left pixel (h,w) against right pixel (h+k, w-d): the 64 rounded products summed
 *                 in NumPy's pairwise order (pf:89), exactly the arithmetic of MCCNN_CV_EXACT; defined for 0 <= w-d,
 *                 w < W and 0 <= h+k < H.
 *   S_L(d,h,w) = max over k = -r..r with 0 <= h+k < H of P(k; d,h,w)                 for w >= d       (left scores)
 *   S_R(d,h,w) = max over k = -r..r with 0 <= h-k < H of P(k; d,h-k,w+d)             for w+d < W      (right scores)
 * S_R matches right pixel (h,w) against left pixel (h-k, w+d): the same pairing seen from the other view.  For r > 0 it
 * is NOT a copy of S_L; for r = 0 it is the reference's copy (pf:104).  Rows outside the image are skipped, not clamped.
 * The maximum: candidates in ascending k; best = the first candidate; then best = s if (s > best or isnan(s)) else best.
 * So a NaN candidate makes the score NaN and it stays NaN, and among equal values (+-0 included) the first one seen is
 * kept.  Then the reference's border recurrences on S_L and S_R (pf:94-95, 105-106) and the negation (pf:111-112): the
 * fill launch of mccnn_cost_volume_hwd, unchanged.  vertical_range = 0 is bit-identical to mccnn_cost_volume_hwd with
 * MCCNN_CV_EXACT (the Dp - D pad entries of a pixel are not written either way).
 * MCCNN_E_INVALID: null pointers, vertical_range outside [0, 4].  MCCNN_E_UNSUPPORTED: outside 2 <= D <= 1024,
 * D <= W - 2, C = 64, one volume row below 2 GiB.  No allocation, no synchronisation: capturable. */
#define MCCNN_VERTICAL_RANGE_MAX 4
int mccnn_cost_volume_vertical_hwd(const float *fl, const float *fr, int H, int W, int C, int D, int vertical_range,
                                   float *lcv_hwd, float *rcv_hwd, mccnn_stream_t stream);

/* ---- a pair's ROW OFFSET: measured on the device, and the cost volume taken along it (not in the reference) ----------
 * A pair whose right image sits k0 rows low needs no search: it needs the volume taken against row h + k0.  P(k; d,h,w)
 * and the maximum rule (ascending order, NaN sticky, the first of equal values kept) are those of
 * mccnn_cost_volume_vertical_hwd above; so are the envelope and the refusals of the two calls that read features.
 *
 * mccnn_vertical_profile: the measurement, for the left view.  R = max_offset, 0 <= R <= 8; row_step >= 1.
 *   profiled rows   h_i = row_step / 2 + i * row_step < H, i = 0 .. n_rows - 1; n_rows = mccnn_vertical_profile_rows(H,
 *                   row_step) (0 where row_step / 2 >= H)
 *   b(k)            for a profiled row h, a pixel w and every k in -R..R with 0 <= h + k < H: the maximum over
 *                   d = 0 .. min(D - 1, w), d ascending, of P(k; d,h,w)
 *   vote            a pixel votes unless one of its b(k) is NaN.  Its winner: best = b(0); then the candidates -1, +1, -2,
 *                   +2, ... in this order, each replacing the best only when strictly greater - ties go to the smaller
 *                   |k|, a flat image votes 0
 *   votes           uint32 [n_rows][ceil(W / 64)][2R + 1]: votes[i][w / 64][winner + R] counts the pixels.  The call
 *                   overwrites all of it (a memset node and one kernel); integer atomics only: deterministic
 * MCCNN_E_INVALID: also max_offset outside [0, 8], row_step < 1.  MCCNN_E_SCRATCH: votes_bytes below the array's size.
 *
 * mccnn_vertical_offset_select: totals[k + R] (uint64 [2R + 1]) = the votes for k over all rows and blocks; *offset
 * (int32) = the k of the largest total, candidates and replacement as for the vote; no votes at all give 0.  votes,
 * offset and totals are device buffers; one small launch.
 *
 * mccnn_cost_volume_offset_hwd: the pixel-major volumes along the offset.  row_offset: a DEVICE int32, read by the
 * kernel (so a measured offset needs no host round trip); k0 = min(max(*row_offset, -8), 8), whatever is stored; a null
 * pointer means 0.  r = vertical_range, 0 <= r <= 4:
 *   S_L(d,h,w) = max over k = k0-r .. k0+r with 0 <= h+k < H of P(k; d,h,w); where no such k exists,
 *                P(kc; d,h,w) with kc = clamp(k0, -h, H-1-h): the nearest image row
 *   S_R(d,h,w) = max over the same k with 0 <= h-k < H of P(k; d,h-k,w+d); where none exists, kc = clamp(k0, h-(H-1), h)
 * then the border recurrences and the negation: the unchanged fill launch.  Pads are not written.  *row_offset = 0 (and
 * a null pointer) give the bits of mccnn_cost_volume_vertical_hwd at the same range.  With a pointer the search kernel
 * runs at every range: 2 (2r + 1) product sets.
 * All three: no allocation, no synchronisation: capturable. */
#define MCCNN_VERTICAL_OFFSET_MAX 8
int mccnn_vertical_profile_rows(int H, int row_step);
int mccnn_vertical_profile(const float *fl, const float *fr, int H, int W, int C, int D, int max_offset, int row_step,
                           uint32_t *votes, size_t votes_bytes, mccnn_stream_t stream);
int mccnn_vertical_offset_select(const uint32_t *votes, int n_rows, int n_blocks, int max_offset, int32_t *offset,
                                 uint64_t *totals, mccnn_stream_t stream);
int mccnn_cost_volume_offset_hwd(const float *fl, const float *fr, int H, int W, int C, int D, const int32_t *row_offset,
                                 int vertical_range, float *lcv_hwd, float *rcv_hwd, mccnn_stream_t stream);

/* ---- a FIELD of row offsets: one per cell of a coarse grid (not in the reference) ---------------------------------------
 * One offset models a right camera that sits low; a rolled rig or two unequal focal lengths leave a residual that grows
 * with the column or with the row and averages to nothing.  P(k; d,h,w), the maximum rule, the vote, the profiled rows
 * h_i and the votes array are those above, untouched.
 *
 * Grid: gh x gw cells, 1 <= gh, gw <= 8, gh <= H, gw <= nb = ceil(W / 64).  Integer divisions throughout:
 *   row band of image row h      h * gh / H
 *   column band of column x      (x / 64) * gw / nb
 * A cell that contains no profiled row has no votes.
 *
 * mccnn_vertical_field_select: votes as written by mccnn_vertical_profile for (H, row_step, R = max_offset); n_rows must
 * be mccnn_vertical_profile_rows(H, row_step), n_blocks = nb.  All outputs are device buffers:
 *   totals          uint64 [gh][gw][2R + 1]: totals[a][b][k + R] = the sum of votes[i][blk][k + R] over the profiled rows
 *                   h_i of row band a and the blocks blk of column band b
 *   field           int32 [gh][gw]: the winner of the cell's totals by the rule of the vote (candidates 0, -1, +1, ...,
 *                   only a strictly greater total replaces); a cell without a single vote takes the global winner
 *   offset, global_totals   int32, uint64 [2R + 1]: exactly what mccnn_vertical_offset_select returns for these votes
 * One small launch, integer atomics only (deterministic), no allocation, no synchronisation: capturable.
 * MCCNN_E_INVALID: a null pointer, max_offset outside [0, 8], row_step < 1, H <= 0, n_rows other than the profile's,
 * n_blocks < 1, gh or gw outside [1, 8], gh > H, gw > n_blocks - each message names its argument.
 *
 * mccnn_cost_volume_field_hwd: the pixel-major volumes along the field.  field: DEVICE int32 [gh][gw], read by the kernel.
 *   F(h, x)    = the word of field at (row band of h, column band of min(x, W - 1)), clamped to +-8 whatever it holds
 *   S_L(d,h,w) = mccnn_cost_volume_offset_hwd's S_L with k0 = F(h, w)
 *   S_R(d,h,w) = its S_R with k0 = F(h, w + d): the cell at the right pixel's own row and at the column of its left
 *                partner, so that both views agree on which left column owns the offset
 * vertical_range and the nearest-image-row rule are applied per entry; then the unchanged fill launch.  Pads are not
 * written.  A field whose cells all hold k gives the bits of mccnn_cost_volume_offset_hwd with *row_offset = k at every
 * range; a 1 x 1 grid is that call.  Refusals as for mccnn_cost_volume_offset_hwd (field must not be null), and
 * MCCNN_E_INVALID for gh or gw outside [1, 8], gw > ceil(W / 64), gh > H; a refused call writes nothing.  Cost: per
 * workgroup and disparity tile one product set for every candidate that one of the tile's entries selects - 2 (2r + 1)
 * sets per pixel where the cells agree, more only along a cell border.  Capturable. */
#define MCCNN_VERTICAL_FIELD_MAX 8
int mccnn_vertical_field_select(const uint32_t *votes, int n_rows, int n_blocks, int H, int row_step, int max_offset, int gh,
                                int gw, int32_t *field, uint64_t *totals, int32_t *offset, uint64_t *global_totals,
                                mccnn_stream_t stream);
int mccnn_cost_volume_field_hwd(const float *fl, const float *fr, int H, int W, int C, int D, const int32_t *field, int gh,
                                int gw, int vertical_range, float *lcv_hwd, float *rcv_hwd, mccnn_stream_t stream);

/* ---- a2 for the "accurate" network (Zbontar & LeCun 2016, sec. 3.2): the decision MLP on the matrix cores -----------
 * s(h,w,d) = sigmoid(wf . relu(W_n ... relu(W_2 . relu(aL[h,w] + aR[h,w-d]) + b_2) ... + b_n) + bf) for w >= d;
 * lcv = -s at (h,w,d), rcv = -s at (h,w-d,d); the border columns are filled by the same recurrences, the same kernels,
 * as mccnn_cost_volume / mccnn_cost_volume_hwd (plane-major [D][H][W] / pixel-major [H][W][Dp]).
 * aL, aR: [H][W][units] float32, the two halves of the first fully-connected layer evaluated per pixel by the caller
 *   (aL = W1[:, :C] . fL + b1, aR = W1[:, C:] . fR: the layer is linear in the concatenation).
 * n_fc: hidden layers of `units` units INCLUDING that first one; the kernel applies layers 2 .. n_fc.
 * packed: their weights as mccnn_decision_pack laid them out for the same n_fc and mode with weight_scale (a power of
 *   two that brings max |w| near 1024); weights: [n_fc-1][units out][units in] float32; biases: [n_fc-1][units];
 *   w_final [units], b_final: the last layer.  mccnn_decision_pack_bytes: size of `packed` (0: outside the envelope).
 *   weight_scale must be positive and FINITE (MCCNN_E_INVALID otherwise, nothing launched, in all three entry points),
 *   and weight_scale * 256 and its reciprocal must be normal float32 numbers: weight_scale in [2^-126, 2^118].
 *   Dynamic range of a caller's own packing: ONE scale serves every layer.  A split operand is w * scale = hi + lo in
 *   f16: |w * scale| > 65504 is clamped; the pair carries 22 bits while |w * scale| >= 0.25, loses bits of `lo`
 *   (an f16 subnormal) below that, is `hi` alone below 2^-13 and 0 below 2^-25.  With max |w| * scale in
 *   (512, 1024] a weight 2^-11 of the largest still has all its bits; a whole LAYER that small next to a larger one
 *   does not, and its error is not flagged.  Bring the layers' largest weights into one binade first - scale
 *   (W_k, b_k) by a power of two c_k and W_k+1 by 1 / c_k, through to w_final: relu(c x) = c relu(x), exact in
 *   float32 - as ACCURATE_NET.decision_layers does.  The activations carry the fixed factor 256 the same way: full
 *   precision for 2^-10 <= x <= 255.875, flagged above, silently coarser below.
 * mode MCCNN_CV_EXACT: every float32 operand as two f16 numbers, three v_mfma_f32_32x32x16_f16 products per multiply,
 *   float32 accumulation - float32-accurate scores; MCCNN_CV_MFMA: one f16 product per multiply.
 * saturation_flag (device int, may be NULL): set to 1 when an activation of a stored voxel (w >= d, d < D, w < W)
 *   exceeds the f16 range of the operands (x * 256 > 65504, +inf included; clamped) or is NaN of either sign - in
 *   aL + aR or in a hidden layer's pre-activation; behind the last hidden layer, which feeds the float32 final
 *   product, NaN alone.  -inf is what relu makes of it, 0, and raises nothing: the library route agrees.  The contract
 *   of mccnn_conv3x3_split; what a flagged call stores in such a voxel is unspecified (finite where the kernel
 *   clamped, never the network's NaN): the flag means "repeat on the library route".  Never cleared by the call.
 * Envelope (MCCNN_E_UNSUPPORTED outside): C (feature maps behind aL / aR) 64 or 112, units = 384, n_fc 3 or 4,
 *   2 <= D <= 1024, D <= W - 2, H <= 65535; _hwd: one volume row below 2 GiB. */
size_t mccnn_decision_pack_bytes(int n_fc, int units, int mode);
int mccnn_decision_pack(const float *weights, int n_fc, int units, float weight_scale, int mode, void *packed,
                        mccnn_stream_t stream);
int mccnn_cost_volume_accurate(const float *aL, const float *aR, int H, int W, int C, int units, int n_fc, int D,
                               const void *packed, const float *biases, const float *w_final, float b_final,
                               float weight_scale, float *lcv, float *rcv, int mode, int *saturation_flag,
                               mccnn_stream_t stream);
int mccnn_cost_volume_accurate_hwd(const float *aL, const float *aR, int H, int W, int C, int units, int n_fc, int D,
                                   const void *packed, const float *biases, const float *w_final, float b_final,
                                   float weight_scale, float *lcv_hwd, float *rcv_hwd, int mode, int *saturation_flag,
                                   mccnn_stream_t stream);

/* The border recurrences alone (pf:94-95, 105-106) on volumes whose w >= d entries are written: the launch every entry
 * point above ends with, for callers that produce the scores themselves (the library route of the accurate network).
 * pixel_major = 0: [D][H][W]; != 0: [H][W][Dp], D <= 1024 and one volume row below 2 GiB. */
int mccnn_cost_volume_fill(float *lcv, float *rcv, int D, int H, int W, int pixel_major, mccnn_stream_t stream);

/* ---- a3  compute_cross_region (pf:571-657) ----------------------------------------------------------------
 * Per pixel: the four arm lengths (<= L-1 per side, anchor-relative threshold |I(q)-I(p)| < tau) and the region
 * size count = sum over the vertical arm of (left+right+1), packed in one 32-bit word so that the aggregation
 * kernel fetches everything about two neighbouring pixels with one 8-byte load:
 *     bits 0-4 up | 5-9 down | 10-14 left | 15-19 right | 20-31 count        (arms <= 31, count <= 63*63)
 * hence L <= 32.  The reference's explicit coordinate list [H][W][(2L)^2][2] (padded with -1) is produced by
 * mccnn_cross_region_list for API compatibility only.
 * The support buffer holds four derived planes behind the first (each 16-byte aligned), private to the kernels
 * of mccnn_cbca_iter / mccnn_cbca_iter_hwd.  Two are written for the streaming kernel's LDS layout: [H][W] uint32 "hsum words" (LDS byte addresses of the two row-prefix
 * entries whose difference is the pixel's horizontal-arm sum) and [H][W] uint64 "emit words" (the float64 reciprocal
 * 1/count with the vertical arms in its 12 low mantissa bits; the 40 upper mantissa bits are chosen so that the word as
 * stored is the float64 nearest to 1/count).  The third lists, for every 16 x 64 pixel tile, its pixels in order of
 * falling region size (uint16 tile-local indices): the order in which the plane-major reference-order kernel deals
 * pixels to lanes, so that a wave's lanes walk regions of similar size.  The fourth, [H][W] uint32 "window masks", is
 * what the pixel-major reference-order kernel (mccnn_cbca_iter_hwd) walks: one bit per column of its register window
 * that the pixel's horizontal arm covers.  Allocate mccnn_support_bytes(H, W) bytes (22 per pixel + alignment) on a
 * 16-byte boundary (memory contract: MCCNN_E_INVALID otherwise, here and in every entry point that takes the buffer);
 * mccnn_cross_arms fills all planes, and consumers that only want the arms / counts read the first H*W words. */
typedef uint32_t mccnn_support_t; /* plane 0 layout [H][W] */
size_t mccnn_support_bytes(int H, int W); /* whole buffer: all planes (0 for non-positive sizes) */
#define MCCNN_SUPPORT_UP(s) ((s) & 31u)
#define MCCNN_SUPPORT_DOWN(s) (((s) >> 5) & 31u)
#define MCCNN_SUPPORT_LEFT(s) (((s) >> 10) & 31u)
#define MCCNN_SUPPORT_RIGHT(s) (((s) >> 15) & 31u)
#define MCCNN_SUPPORT_COUNT(s) ((s) >> 20)
int mccnn_cross_arms(const float *image, int H, int W, float tau, int L, mccnn_support_t *support,
                     mccnn_stream_t stream);
/* Both views in one call (compute_cross_region is called once per image right after each other, pf:120-121): the
 * same results as two mccnn_cross_arms calls, half the launches. */
int mccnn_cross_arms_pair(const float *image_left, const float *image_right, int H, int W, float tau, int L,
                          mccnn_support_t *support_left, mccnn_support_t *support_right, mccnn_stream_t stream);
/* region: [H][W][(2L)^2][2] int32.  L must not be smaller than the distance the plane was built with (a pixel's list
 * would overrun its (2L)^2 slots): like the aggregation entry points, a plane this library built with longer arms or
 * for another image size is refused (MCCNN_E_INVALID); addresses it has never seen pass. */
int mccnn_cross_region_list(const mccnn_support_t *support, int H, int W, int L, int32_t *region,
                            mccnn_stream_t stream);

/* ---- a4  cost_volume_aggregation, ONE iteration on ONE volume (pf:149-163) -----------------------------------
 * out[d,p] = (sum_{q in U(p)} in[d,q]) / count[p];  in != out (ping-pong; the reference does not mutate either).
 * L is the distance threshold the support plane was built with (arms < L; supported: L <= 32); a plane that this
 * library's mccnn_cross_arms built with a larger distance, or for another image size, is refused (MCCNN_E_INVALID).
 * order MCCNN_CBCA_SEPARABLE: horizontal-arm sums then vertical-arm sums.  For L <= 14 they are evaluated through
 * float64 prefix sums: the correctly rounded region mean - |out - exact mean| <= half a float32 spacing of the mean
 * + 2^-34 max|in| - within <= 1e-6 per iteration (O(1) costs) of the reference's sequential float32 sum, cost
 * independent of the arm lengths; volumes must be finite (an inf/nan would poison its whole row).  For 15 <= L <= 32
 * the arms are summed in plain float32 (up to 63 + 63 sequential additions): NOT correctly rounded,
 * |out - exact mean| <= (n_h + n_v + 2) 2^-24 (sum over the region of |in|) / count, n_h the longest horizontal span
 * in the region and n_v its vertical span (measured: up to 8 spacings of the mean on costs of one sign).
 * MCCNN_CBCA_REFERENCE_ORDER: the reference's flat running sum (vertical arm self,up..,down.. x horizontal arm
 * self,left..,right..), bit-exact, slower. */
#define MCCNN_CBCA_SEPARABLE 0
#define MCCNN_CBCA_REFERENCE_ORDER 1
int mccnn_cbca_iter(const float *in, float *out, const mccnn_support_t *support, int D, int H, int W, int L, int order,
                    mccnn_stream_t stream);

/* One iteration on the left AND the right volume (same D, H, W; each with its own support planes) - the reference's
 * cost_volume_aggregation takes both views in one call (match.py:142, 154; pf:116-180 loops over the two).  Same
 * results as two mccnn_cbca_iter calls; for MCCNN_CBCA_SEPARABLE with L <= 14 it is ONE launch whose workgroups are dealt
 * the work of both volumes (fewer, fuller rounds: 750x500x256 is exactly three rounds of 256 workgroups), every
 * other variant runs the two single-volume launches. */
int mccnn_cbca_iter_pair(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                         const float *in_right, float *out_right, const mccnn_support_t *support_right, int D, int H,
                         int W, int L, int order, mccnn_stream_t stream);

/* The paper's support regions from BOTH views (sec. 4.1; the reference skips it, pf:122-144, 661-729 dead code).
 * Opt-in, changes the output: at disparity d every arm used at a pixel q is min(own arm at q, the other view's arm at
 * the partner q -/+ d) (side LEFT: x - d, RIGHT: x + d; partner outside the image: own arms).  Flat float32 running
 * sum in the reference's order, region size counted on the way.  support_self / support_other: planes built by
 * mccnn_cross_arms on the volume's own view and on the other view.  Own arms are first clamped to R (13 for L <= 14,
 * 31 above), then intersected.  Refused: in == out, a side other than MCCNN_SIDE_LEFT / _RIGHT (MCCNN_E_INVALID); L
 * outside [1,32], D > 65535 (MCCNN_E_UNSUPPORTED); and, as in mccnn_cbca_iter, either plane when this library built it
 * for another image size or with a distance larger than L (MCCNN_E_INVALID).  Addresses it has never seen pass: for
 * those the clamp to R is what keeps every read inside the staged tile. */
int mccnn_cbca_iter_both(const float *in, float *out, const mccnn_support_t *support_self,
                         const mccnn_support_t *support_other, int D, int H, int W, int L, int side,
                         mccnn_stream_t stream);

/* ---- a4 on the pixel-major layout: ONE iteration in the reference's summation order, bit-exact (pf:149-163) ----
 * in_hwd / out_hwd are "HWD" volumes [H][W][Dp]; out[p,d] = the reference's flat float32 running sum over the region
 * list of p (vertical arm self,up..,down.. x horizontal arm self,left..,right..) divided by count[p].  A wave owns a
 * few neighbouring pixels and all their disparities (disparities on lanes), so the region walk runs on the scalar
 * unit and every region element is one coalesced load: same bits as mccnn_cbca_iter(..., MCCNN_CBCA_REFERENCE_ORDER)
 * on the plane-major volume, an order of magnitude faster.  The kernel reads plane 0 of the support buffer AND its
 * window-mask plane (one word per pixel, behind the derived planes): `support` must be the start of the WHOLE
 * mccnn_support_bytes(H, W) buffer that mccnn_cross_arms wrote - a copy of plane 0 alone is refused
 * (MCCNN_E_INVALID: the *_hwd entry points only accept pointers mccnn_cross_arms has written).  L <= 14; in != out.
 * The _pair form takes the left and the right volume in one launch (pf:116-180 loops over the two views). */
int mccnn_cbca_iter_hwd(const float *in_hwd, float *out_hwd, const mccnn_support_t *support, int D, int H, int W, int L,
                        mccnn_stream_t stream);
int mccnn_cbca_iter_hwd_pair(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                             const float *in_right, float *out_right, const mccnn_support_t *support_right, int D,
                             int H, int W, int L, mccnn_stream_t stream);

/* The LAST iteration of an aggregation fused with a7 (pf:239-272): like mccnn_cbca_iter_hwd_pair, and the first strict
 * minimum over d of every pixel of the two results goes to disparity_left / disparity_right ([H][W] float32, -1 where
 * no disparity wins), exactly what mccnn_wta_hwd returns on the stored volumes.  store_right = 0 leaves out_right
 * unwritten (it may then be NULL): match.py needs the final right volume for nothing but its WTA.  One chunk of
 * disparities per wave: D <= 256 (MCCNN_E_UNSUPPORTED beyond; run mccnn_wta_hwd then). */
int mccnn_cbca_iter_hwd_pair_wta(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                                 const float *in_right, float *out_right, const mccnn_support_t *support_right, int D,
                                 int H, int W, int L, float *disparity_left, float *disparity_right, int store_right,
                                 mccnn_stream_t stream);

/* ---- a4 on the pixel-major layout for every distance the support word holds: 1 <= L <= 32 (arms up to 31) ----------
 * Same contract and same bits as mccnn_cbca_iter_hwd / mccnn_cbca_iter_hwd_pair (whole support buffer written by
 * mccnn_cross_arms, in != out, no allocation, no synchronisation, D up to 1024), with a register window of 2 pixels x
 * 63 columns and 128-disparity chunks instead of 5 x 27 and 256: for L <= 14 the result equals mccnn_cbca_iter_hwd's
 * bit for bit, for 15 <= L <= 32 it equals mccnn_cbca_iter(..., MCCNN_CBCA_REFERENCE_ORDER) on the plane-major volume.
 * Only plane 0 of the support buffer is read (the window masks are derived from its arm fields).  L > 32:
 * MCCNN_E_UNSUPPORTED.  The input is addressed row by row, so the shape limit is one image row below 2 GiB.  There is
 * no fused-WTA form: run mccnn_wta_hwd on the result of the last iteration. */
int mccnn_cbca_iter_hwd_long(const float *in_hwd, float *out_hwd, const mccnn_support_t *support, int D, int H, int W,
                             int L, mccnn_stream_t stream);
int mccnn_cbca_iter_hwd_long_pair(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                                  const float *in_right, float *out_right, const mccnn_support_t *support_right, int D,
                                  int H, int W, int L, mccnn_stream_t stream);

/* ---- a4 on the pixel-major layout, program-driven (pf:149-163; round 4) ---------------------------------------------
 * Bit-identical to mccnn_cbca_iter_hwd_pair and faster (0.45 vs 0.55 ms per two-volume iteration at 750x500x256): the
 * per-image control of that kernel - region rows, pixel windows and arm runs of every 4 x 5 patch of anchors - is
 * compiled once per image into a linear program per patch (mccnn_cbca_prog_build_pair, after mccnn_cross_arms), and the
 * iteration is an interpreter of those programs written in gfx950 assembly (csrc/asm/cbca_prog_gen.py).  The programs
 * depend on the image, on D (disparities per lane) and on nothing else: one build serves all 18 iterations of a pair.
 *   mccnn_cbca_prog_bytes: size of ONE image's program buffer, which must be 16-byte aligned (memory contract:
 *     MCCNN_E_INVALID otherwise, in the builders and in every launch) (room for two program sets: the full programs and the
 *     ones mccnn_cbca_iter_prog_pair_skip runs); 0 when the shape is outside what the programs encode
 *     (W > 2180 columns, or volumes beyond a buffer descriptor's reach) - callers then stay with mccnn_cbca_iter_hwd_pair.
 *   support_*: the whole buffers mccnn_cross_arms wrote (plane 0 is read).  L <= 14; outputs must not alias inputs.
 *   mccnn_cbca_iter_prog_pair refuses (MCCNN_E_INVALID) program buffers mccnn_cbca_prog_build_pair has not written, built
 *   for another shape, or built from support arms that mccnn_cross_arms has overwritten since: the kernel follows its
 *   programs blindly. */
size_t mccnn_cbca_prog_bytes(int D, int H, int W);
int mccnn_cbca_prog_build_pair(const mccnn_support_t *support_left, const mccnn_support_t *support_right, int D, int H,
                               int W, int L, void *prog_left, void *prog_right, mccnn_stream_t stream);
int mccnn_cbca_iter_prog_pair(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                              const void *prog_left, const float *in_right, float *out_right,
                              const mccnn_support_t *support_right, const void *prog_right, int D, int H, int W, int L,
                              mccnn_stream_t stream);
/* The last iteration fused with a7 (pf:239-272), like mccnn_cbca_iter_hwd_pair_wta: also writes the first strict minimum
 * over d of both results to disparity_left / disparity_right ([H][W] float32, -1 where nothing wins); store_right = 0
 * leaves out_right unwritten (it may then be NULL).  One chunk of disparities per wave: D <= 256. */
int mccnn_cbca_iter_prog_pair_wta(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                                  const void *prog_left, const float *in_right, float *out_right,
                                  const mccnn_support_t *support_right, const void *prog_right, int D, int H, int W, int L,
                                  float *disparity_left, float *disparity_right, int store_right, mccnn_stream_t stream);

/* A later iteration of the SAME ping-pong pair of buffers, without the pixels that cannot change any more.  A pixel
 * whose support region is the pixel itself (all four arms 0: count 1) gets v1 = (0 + v0) / 1 in the first iteration
 * (pf:156-161) - v0 except that -0.0 becomes +0.0 and a signalling NaN is quieted - and (0 + v1) / 1 = v1 bit for bit
 * ever after.  This entry point may replace mccnn_cbca_iter_prog_pair from the SECOND consecutive iteration on: it runs
 * the second program set, which mccnn_cbca_prog_build_skip_pair writes into the same buffers (a launch of its own, so
 * that it can run beside the first iterations); such anchors take no part - not loaded for their own sake, not divided,
 * NOT STORED (on the synthetic benchmark pair 46 % of the pixels: 27 % less HBM traffic per iteration).  What the
 * caller must know: out_* keeps, for every such pixel, what it held before.  After a first full iteration in -> out
 * that is v1 in `out` and still v0 in `in`; as an operand of somebody else's sum the two are interchangeable (a sum
 * that began as 0 + x is never -0.0, so adding -0.0 or +0.0 gives the same bits; either NaN gives the same quiet NaN),
 * but a caller that READS such a pixel from the buffer that was the first iteration's input must first run one full
 * iteration into it.  match.py's 16-iteration aggregation (pf:117-183 with max_average_time = 16) therefore runs
 * iteration 1 full, iterations 2 .. 15 this way, and the last one - which carries the WTA and writes every pixel
 * into the first iteration's input buffer - full again (stereo_device.cbca_prog_pair states the rule for any count). */
int mccnn_cbca_prog_build_skip_pair(const mccnn_support_t *support_left, const mccnn_support_t *support_right, int D,
                                    int H, int W, int L, void *prog_left, void *prog_right, mccnn_stream_t stream);
/* Both program sets from ONE pass over the support words (round 5): what mccnn_cbca_prog_build_pair followed by
 * mccnn_cbca_prog_build_skip_pair write, word for word, in one launch and about half their time (the sweep steps of the
 * two programs of a patch share a wave's lanes). */
int mccnn_cbca_prog_build_both_pair(const mccnn_support_t *support_left, const mccnn_support_t *support_right, int D,
                                    int H, int W, int L, void *prog_left, void *prog_right, mccnn_stream_t stream);
int mccnn_cbca_iter_prog_pair_skip(const float *in_left, float *out_left, const mccnn_support_t *support_left,
                                   const void *prog_left, const float *in_right, float *out_right,
                                   const mccnn_support_t *support_right, const void *prog_right, int D, int H, int W,
                                   int L, mccnn_stream_t stream);

/* One volume per launch (round 5): the same kernels with half the grid.  A stereo pair's two volumes are independent
 * chains of iterations; issued as two such chains on two streams, one chain's launch fills the compute units that the
 * other chain's launch leaves idle while its last and heaviest patches finish (the skip launches, whose work sits in a
 * few image regions, end with most of the chip idle): 8.7 % less time for 16 iterations at 750x500x256 than one
 * two-volume launch per iteration, same bits.  `prog` is one image's buffer as mccnn_cbca_prog_build_pair /
 * _build_skip_pair wrote it (either position of the pair); the same refusals as the two-volume entry points. */
int mccnn_cbca_iter_prog(const float *in, float *out, const mccnn_support_t *support, const void *prog, int D, int H, int W,
                         int L, mccnn_stream_t stream);
int mccnn_cbca_iter_prog_skip(const float *in, float *out, const mccnn_support_t *support, const void *prog, int D, int H,
                              int W, int L, mccnn_stream_t stream);

/* The FIRST iteration of an aggregation whose later iterations run the skip programs (round 6): exactly
 * mccnn_cbca_iter_prog(_pair) - the full programs, every pixel of `out` written - and, besides, the value v1 = (0 + v0) / 1
 * of every unit-region pixel is written back into `in` (pf:156-161 with aver_num = 1: `in` is NOT const here).  After
 * it both buffers of the ping-pong pair hold v1 at those pixels, so EVERY later iteration may be a _skip launch,
 * whichever buffer the last one writes: without it `in` keeps v0, which differs from v1 where v0 is -0.0, and an
 * aggregation with an even number of iterations (match.py's first: 2) had to end with a full launch.  Waves that read
 * such a pixel as a neighbour while it is being rewritten see v0 or v1 - as an operand the two give the same bits (see
 * above), so the race cannot be observed.  Same programs, same refusals as mccnn_cbca_iter_prog(_pair). */
int mccnn_cbca_iter_prog_refresh(float *in, float *out, const mccnn_support_t *support, const void *prog, int D, int H, int W,
                                 int L, mccnn_stream_t stream);
int mccnn_cbca_iter_prog_pair_refresh(float *in_left, float *out_left, const mccnn_support_t *support_left,
                                      const void *prog_left, float *in_right, float *out_right,
                                      const mccnn_support_t *support_right, const void *prog_right, int D, int H, int W,
                                      int L, mccnn_stream_t stream);

/* ---- layout changes between DHW and HWD -------------------------------------------------------------------
 * Any 4-byte-aligned bases (the 16-byte transposes run only between two 16-byte-aligned ones, same bits).  mccnn_dhw_to_hwd
 * leaves the pad entries of hwd unspecified; mccnn_hwd_to_dhw never copies one. */
int mccnn_hwd_pitch(int D); /* Dp: D rounded up to a multiple of 4 (16-byte rows) */
int mccnn_dhw_to_hwd(const float *dhw, float *hwd, int D, int H, int W, mccnn_stream_t stream);
int mccnn_hwd_to_dhw(const float *hwd, float *dhw, int D, int H, int W, mccnn_stream_t stream);

/* ---- a6  semi_global_matching, one axis-aligned direction, in place (pf:476-568) -----------------------------
 * vol_hwd is updated in place along r = (rh, rw) in {(0,1),(0,-1),(-1,0),(1,0)}; the first line of the scan
 * axis is left untouched.  Penalties are recomputed from the two images (no P1/P2/D2 volumes):
 *   (P1,P2) = (p1,p2) if D1<thr and D2<thr; /q2 if both >= thr; /q1 otherwise      (pf:535-541)
 * p1, p2, q1, q2, thr are the float32 roundings NumPy applies to the Python scalars (pass float(sgm_P1/sgm_V)
 * as p1 for the vertical directions, pf:204).  float32 add/min/sub only, un-fused: bit-exact vs the reference.
 * Up to two volumes (e.g. left + right) are advanced by one launch so the chip sees 2x the scanlines:
 * n_jobs in {1,2}; job j updates vol_hwd[j] as side[j].  scratch >= mccnn_sgm_scratch_bytes(H,W,D). 2<=D<=1024.
 * scratch / flags of every SGM entry point: 16-byte aligned (memory contract: MCCNN_E_SCRATCH otherwise).  The pad entries
 * of vol_hwd are read, masked to +inf, and overwritten with unspecified values; they never reach an entry d < D.
 * No limit on the volume's size: vertical scanlines of volumes of 4 GiB or more run a variant that rebases its buffer
 * descriptor every few steps (same bits). */
size_t mccnn_sgm_scratch_bytes(int H, int W, int D);
int mccnn_sgm_pass(const float *image_left, const float *image_right, float *const *vol_hwd, const int *side,
                   int n_jobs, int D, int H, int W, int rh, int rw, float p1, float p2, float q1, float q2, float thr,
                   void *scratch, size_t scratch_bytes, mccnn_stream_t stream);
/* The two halves of mccnn_sgm_pass as calls of their own (ABI 7, round 6).  The flag planes (pf:504-533: which pixels'
 * intensity step along r reaches thr) depend on the two images, r and thr only: mccnn_sgm_flags writes them into `flags`
 * (>= mccnn_sgm_scratch_bytes(H,W,D)), mccnn_sgm_pass_flagged is the pass itself on planes built for the same H, W, D
 * and r.  A caller that advances the two volumes of a pair in separate launches (StereoMatcher: two free-running chains
 * on two streams) builds the planes of each direction once, off the critical path, and both chains read them. */
int mccnn_sgm_flags(const float *image_left, const float *image_right, int D, int H, int W, int rh, int rw, float thr,
                    void *flags, size_t flags_bytes, mccnn_stream_t stream);
int mccnn_sgm_pass_flagged(float *const *vol_hwd, const int *side, int n_jobs, int D, int H, int W, int rh, int rw, float p1,
                           float p2, float q1, float q2, const void *flags, size_t flags_bytes, mccnn_stream_t stream);

/* The out-of-place, accumulating form of the pass: the paper's SGM, C_SGM = 1/4 sum_r L_r with every L_r computed from
 * the SAME volume (the reference's SGM_average composes its four passes on one aliased array instead, pf:195-210; see
 * StereoMatcher's extra sgm_independent_directions).  Job j reads its costs from src_hwd[j], which is never written,
 * runs the recurrence of mccnn_sgm_pass along r in registers, and combines every line of L - the first line of the
 * scan axis, where L = C, included - with acc_hwd[j] (same [H,W,Dp] layout):
 *   MCCNN_SGM_ACC_STORE        acc  = L                       (what acc held is not read)
 *   MCCNN_SGM_ACC_ADD          acc  = acc + L                 float32
 *   MCCNN_SGM_ACC_ADD_QUARTER  acc  = (acc + L) / 4.f         float32, correctly rounded
 * so store, add, add, add-and-quarter over the reference's four directions give (((L0 + L1) + L2) + L3) / 4.  An axis
 * with a single line contributes L = C.  flags: mccnn_sgm_flags for the same H, W, D and r.  Refused (MCCNN_E_INVALID):
 * null pointers, an unknown mode, an r that is not an axis-aligned unit step, and any overlap between an accumulator and
 * a source or another accumulator; 2 <= D <= 1024 (MCCNN_E_UNSUPPORTED), flags_bytes >= mccnn_sgm_scratch_bytes
 * (MCCNN_E_SCRATCH).  Every route of mccnn_sgm_pass, vertical scanlines of volumes of 4 GiB or more included. */
#define MCCNN_SGM_ACC_STORE 0
#define MCCNN_SGM_ACC_ADD 1
#define MCCNN_SGM_ACC_ADD_QUARTER 2
int mccnn_sgm_pass_accumulate(const float *const *src_hwd, float *const *acc_hwd, const int *side, int n_jobs, int D, int H,
                              int W, int rh, int rw, float p1, float p2, float q1, float q2, int mode, const void *flags,
                              size_t flags_bytes, mccnn_stream_t stream);

/* The first direction of SGM_average, r = (0,1) (pf:194-195, 216-217), fused with the layout change: reads the
 * plane-major volumes vol_dhw[j] (left untouched) and writes the pixel-major vol_hwd[j], i.e. it replaces
 * mccnn_dhw_to_hwd + mccnn_sgm_pass(rh=0, rw=1) and saves one full read + write of every volume.  2 <= D <= 256.
 * Volumes of 4 GiB or more (beyond the reach of the fused gather) run as exactly those two calls: same result. */
int mccnn_sgm_first_pass(const float *image_left, const float *image_right, const float *const *vol_dhw,
                         float *const *vol_hwd, const int *side, int n_jobs, int D, int H, int W, float p1, float p2,
                         float q1, float q2, float thr, void *scratch, size_t scratch_bytes, mccnn_stream_t stream);

/* ---- a7  disparity_prediction, one volume (pf:239-272): first strict minimum over d, as float32 --------------
 * A pixel whose D costs are all NaN / +inf gets -1 (the reference asserts there, pf:253); mccnn_lr_status treats a
 * disparity <= -1 or NaN as an occlusion. */
int mccnn_wta(const float *vol_dhw, int D, int H, int W, float *disparity, mccnn_stream_t stream);

/* The same on a pixel-major volume [H][W][Dp] (one 1 KiB run per pixel at D = 256): same index, same -1 rule. */
int mccnn_wta_hwd(const float *vol_hwd, int D, int H, int W, float *disparity, mccnn_stream_t stream);

/* ---- a8  interpolation (pf:279-378) -------------------------------------------------------------------------
 * mccnn_lr_status: 0 match, 1 mismatch, 2 occlusion (pf:285-307).  A left disparity is truncated toward zero (pf:287:
 * values in (-1, 0) count as 0); one that is <= -1 or NaN, which the reference cannot index, is an occlusion.  Right
 * disparities may hold anything (NaN, +-inf, negative, >= D match nothing).  Rows wider than 16384 pixels put the image
 * rows on grid.y: H <= 65535 there (MCCNN_E_UNSUPPORTED beyond).
 * mccnn_interpolate: status 1 -> median (np.median: a median of -0.0 is +0.0) of the nearest status-0 pixel
 * right/left/below/above, status 2 -> nearest status-0 pixel to the right, else raw.  As in np.median, one NaN among
 * the neighbours makes the median NaN (the status map is the caller's: mccnn_lr_status never marks a NaN disparity as a
 * match, other status maps may); any status word other than 0 is "no match", other than 1 / 2 leaves the raw value.
 * The same holds for mccnn_interpolate_ex.  `out` must alias neither
 * disp_left nor status (MCCNN_E_INVALID: other threads still read both); H <= 65535 (MCCNN_E_UNSUPPORTED beyond), also
 * for mccnn_interpolate_ex. */
int mccnn_lr_status(const float *disp_left, const float *disp_right, int H, int W, int D, int32_t *status,
                    mccnn_stream_t stream);
int mccnn_interpolate(const float *disp_left, const int32_t *status, int H, int W, float *out,
                      mccnn_stream_t stream);
/* The two rules of the paper that the reference names and leaves out (pf:318, pf:361), opt-in: directions = 16 takes
 * the median of the nearest matches along 16 rays instead of the 4 axis directions; occlusion_from_left = 1 fills an
 * occlusion from the nearest match to its left instead of its right.  (4, 0) == mccnn_interpolate. */
int mccnn_interpolate_ex(const float *disp_left, const int32_t *status, int H, int W, int directions,
                         int occlusion_from_left, float *out, mccnn_stream_t stream);

/* ---- a8 for the RIGHT view: the consistency check and the interpolation of the right disparity map ------------------
 * Definition (binding): what mccnn_lr_status / mccnn_interpolate_ex give on the horizontally flipped pair, flipped back.
 * With F(a) = a[:, ::-1]:  status_R = F(lr_status(F(disp_right), F(disp_left), D)),
 *                          interp_R = F(interpolate_ex(F(disp_right), F(status_R), directions, occlusion_from_right)).
 * In image coordinates, for a right pixel (h, x) with rf = disp_right[h][x] and rd = (int)rf (truncated, pf:287):
 *   occlusion (2) if !(rf > -1) or x + rd > W-1;  match (0) if |rd - disp_left[h][x+rd]| <= 1;  mismatch (1) if some d
 *   in 0 .. min(W-x, D)-1 has |d - disp_left[h][x+d]| <= 1, else occlusion (2).  The predicate is the float32 expression
 *   of mccnn_lr_status; the left map may hold anything.  Rows wider than 16384 pixels: H <= 65535, as there.
 * mccnn_interpolate_right: status 1 -> np.median (the -0.0 -> +0.0 and NaN rules of mccnn_interpolate) of the nearest
 *   status-0 pixel left/right/below/above; status 2 -> the nearest status-0 pixel to the LEFT (the mirror of the
 *   reference's "right"), with occlusion_from_right = 1 (the matcher's occlusion_from_left extra, mirrored) to the RIGHT;
 *   else raw.  directions = 16: the mirrored ray set - steps of (-dx, dy) for the 16 (dx, dy) of mccnn_interpolate_ex, in
 *   that order; the column of step k is ceil(x - k*dx - 0.5), i.e. positions round half DOWN along x (half up in the
 *   flipped frame), the row floor(y + k*dy + 0.5) as before.  Any status word other than 0 is "no match", other than
 *   1 / 2 leaves the raw value.  `out` must alias neither disp_right nor status (MCCNN_E_INVALID); H <= 65535
 *   (MCCNN_E_UNSUPPORTED beyond); directions other than 4 / 16: MCCNN_E_INVALID.  (4, 0) runs without per-pixel walks,
 *   like mccnn_interpolate. */
int mccnn_lr_status_right(const float *disp_right, const float *disp_left, int H, int W, int D, int32_t *status,
                          mccnn_stream_t stream);
int mccnn_interpolate_right(const float *disp_right, const int32_t *status, int H, int W, int directions,
                            int occlusion_from_right, float *out, mccnn_stream_t stream);

/* ---- a9  subpixel_enhance (pf:381-400), float32 as NumPy 2 evaluates it ------------------------------------- */
int mccnn_subpixel(const float *disp, const float *vol_dhw, int D, int H, int W, float *out, mccnn_stream_t stream);
/* numpy1_promotion = 1: the scalar promotion of NumPy < 2 (the reference's own Python 2.7 environment): the
 * denominator, the quotient and the subtraction of pf:396 run in float64 and are rounded once on the store;
 * differs from the default by <= 2.5e-5 px.  0 == mccnn_subpixel (what the golden vectors pin). */
int mccnn_subpixel_ex(const float *disp, const float *vol_dhw, int D, int H, int W, int numpy1_promotion, float *out,
                      mccnn_stream_t stream);

/* mccnn_subpixel_ex on a pixel-major volume [H][W][Dp]: the same arithmetic, three neighbouring floats per pixel. */
int mccnn_subpixel_hwd(const float *disp, const float *vol_hwd, int D, int H, int W, int numpy1_promotion, float *out,
                       mccnn_stream_t stream);

/* ---- confidence measures of the left disparity: how far each pixel of the map can be trusted -------------------------
 * One more streaming read of the final aggregated left volume (4 B/voxel, whichever measures are asked for); MSM, MMN
 * and CUR need that volume alone, LRC the right winner-take-all map besides.  Larger always means more confident.
 * Definitions (binding).  For one pixel (h, w) let c[d], 0 <= d < D, be its float32 costs in the final left volume; in
 * the pixel-major layout the pad lanes D <= d < Dp are never read.
 *   d1, c1: best = +inf, d1 = -1; for d ascending: if c[d] < best then best = c[d], d1 = d.  This is exactly mccnn_wta:
 *     NaN and +inf never win.  c1 = c[d1].
 *   No winner: if d1 == -1, every requested plane gets -inf (bits 0xFF800000).
 *   c2: the same scan from +inf over d != d1, value only: an equal cost at a later index gives c2 == c1; +inf if nothing
 *     else is below +inf.
 *   MCCNN_CONF_MSM = 1: -c1 (a sign flip).
 *   MCCNN_CONF_MMN = 2: c2 - c1, one float32 subtraction.
 *   MCCNN_CONF_CUR = 4: cm = d1 >= 1 ? c[d1-1] : c[d1+1];  cp = d1 <= D-2 ? c[d1+1] : c[d1-1];
 *     t = 2.0f * c1;  u = cp - t;  cur = u + cm: three float32 operations in the order of subpixel_hwd_kernel's
 *     denominator; there is no contraction (the library is built with -ffp-contract=off).
 *   MCCNN_CONF_LRC = 8: x = w - d1; if x < 0 the value is -inf.  Otherwise r = disp_right[h*W + x]; if !(r >= 0.0f) ||
 *     r == +inf the value is -inf (that covers NaN, -1 and every negative value; -0.0 passes).  Otherwise the value is
 *     -fabsf((float)d1 - r).
 *   Whatever IEEE arithmetic yields for +-inf costs is the definition (c1 = c2 = -inf gives NaN for MMN).
 * Planes are written in ascending bit order into out[K][H][W], K = popcount(measures); unrequested planes do not exist.
 * One launch, no scratch, no atomics, no synchronisation: capturable.
 * Refused before any HIP call (MCCNN_E_INVALID): null vol / out, D < 2, non-positive H or W, measures == 0 or bits above
 *   15, MCCNN_CONF_LRC with a null disp_right, out overlapping disp_right; for the pixel-major entry D > 1024
 *   (MCCNN_E_UNSUPPORTED, the envelope's limit).
 * Out of scope: measures that need the right volume (the left-right difference: the fused winner-take-all launch leaves
 *   that volume unwritten); measures that need exp (likelihood, entropy: not definable to the bit); the ratio measures
 *   (these costs are negative); the local-minimum margin (after SGM and 16 aggregation iterations the curves are
 *   unimodal: +inf for half the pixels of the reference's own volumes). */
#define MCCNN_CONF_MSM 1u
#define MCCNN_CONF_MMN 2u
#define MCCNN_CONF_CUR 4u
#define MCCNN_CONF_LRC 8u
int mccnn_confidence_hwd(const float *vol_hwd /* [H][W][Dp] */, const float *disp_right /* NULL unless LRC */, int D,
                         int H, int W, unsigned measures, float *out, mccnn_stream_t stream);
int mccnn_confidence(const float *vol_dhw /* [D][H][W] */, const float *disp_right /* NULL unless LRC */, int D, int H,
                     int W, unsigned measures, float *out, mccnn_stream_t stream);

/* The same measures of the RIGHT disparity, from the final aggregated right volume: MSM, MMN and CUR by the definitions
 * above on that volume, unchanged.  LRC: x = w + d1; if x > W-1 the value is -inf.  Otherwise l = disp_left[h*W + x];
 * if !(l >= 0.0f) || l == +inf the value is -inf.  Otherwise the value is -fabsf((float)d1 - l).  The same refusals, with
 * disp_left in the place of disp_right. */
int mccnn_confidence_right_hwd(const float *vol_right_hwd /* [H][W][Dp] */, const float *disp_left /* NULL unless LRC */,
                               int D, int H, int W, unsigned measures, float *out, mccnn_stream_t stream);
int mccnn_confidence_right(const float *vol_right_dhw /* [D][H][W] */, const float *disp_left /* NULL unless LRC */, int D,
                           int H, int W, unsigned measures, float *out, mccnn_stream_t stream);

/* ---- semi-dense maps: selection by validity, left-right status and confidence; speckle filter --------------------------
 * Definitions (binding).
 *   Valid: a disparity is valid when it is finite and >= 0 (mccnn_evaluate's rule): -0.0f is valid; -1, NaN, +-inf are not.
 *   Dropped: a dropped pixel holds +inf (bits 0x7F800000, Middlebury's "unknown"); a kept pixel keeps its bits.  An output
 *     holds nothing else: an input pixel that was already invalid comes out as +inf.
 * mccnn_semi_dense_select, one launch.  A pixel is kept when all of these hold: it is valid; if require_match is set, its
 *   status word is 0 (the plane mccnn_lr_status wrote for the left view, mccnn_lr_status_right for the right one); for
 *   every bit b of `use`, plane_b[h][w] >= min_conf[b] - one float32 compare: a NaN plane value fails, -inf fails every
 *   finite threshold.  planes is [K][H][W] in ascending bit order of plane_measures, exactly what mccnn_confidence* wrote;
 *   `use` must be a subset of plane_measures; min_conf is a HOST array of four floats indexed by bit, read at call time
 *   and passed by value (entries outside `use` are not read); a NaN threshold is refused.  out overlaps no input.
 * Components and mccnn_speckle_filter.  Two 4-neighbours p and q are linked when both are valid and
 *   fabsf(disp[p] - disp[q]) <= max_diff: one float32 subtraction, an inclusive compare.  A component is a class of the
 *   transitive closure of the links (a chain a-b-c is one component even when |a - c| > max_diff); diagonal neighbours
 *   never link; an invalid pixel belongs to no component and has size 0.  sizes[h][w]: the number of pixels of the
 *   pixel's component, uint32.  out[h][w] = disp[h][w] when that size is >= min_size, +inf otherwise.
 *   max_diff >= 0 and not NaN (+inf allowed); min_size >= 1 (1 drops nothing that is valid); out and sizes may each be
 *   NULL, not both; H*W <= 2^31 - 1, beyond that MCCNN_E_UNSUPPORTED.  scratch: mccnn_speckle_scratch_bytes(H, W) bytes,
 *   16-byte aligned, private to one call in flight; the call clears what it needs of it on the stream, so calls may follow
 *   each other on one scratch.
 *   Four launches whose number and sizes depend on H and W alone, no read-back, no allocation, no synchronisation, and no
 *   wait on another workgroup: capturable, and the outputs are a function of the map alone (integer minima and sums).
 *   Rows are not put on grid.y: neither wide rows nor H > 65535 take another path.
 * The rule of a semi-dense map is sparse = speckle_filter(select(map)): components are taken over the pixels that
 *   survived the selection.
 * Refused before any HIP call (MCCNN_E_INVALID): null required pointers, non-positive sizes, `use` not a subset of
 *   plane_measures or bits above 15, require_match with a null status, overlapping output, a scratch that overlaps a
 *   map; a misaligned or short scratch is MCCNN_E_SCRATCH.  A refused call writes nothing. */
int mccnn_semi_dense_select(const float *disp, const int32_t *status /* NULL unless require_match */,
                            const float *planes /* [K][H][W]; NULL allowed when use == 0 */, int H, int W,
                            unsigned plane_measures, unsigned use, const float *min_conf /* host [4] */, int require_match,
                            float *out, mccnn_stream_t stream);
size_t mccnn_speckle_scratch_bytes(int H, int W);   /* 0 for non-positive sizes and beyond the pixel limit */
int mccnn_speckle_filter(const float *disp, int H, int W, float max_diff, unsigned min_size, float *out /* or NULL */,
                         uint32_t *sizes /* or NULL */, void *scratch, size_t scratch_bytes, mccnn_stream_t stream);

/* ---- metric outputs: the depth plane and the ordered point cloud of a disparity map (csrc/reproject.hip) ---------------
 * Still ABI version 7: purely additive, nothing that existed changed.
 * Definitions (binding).  The relation is Middlebury 2014's, Z = baseline * f / (d + doffs), Z in the unit of the
 *   baseline.  All arithmetic is float32 and every operation below is one correctly rounded IEEE operation, never fused,
 *   never a reciprocal.  The caller rounds the host scalars once from float64: fb = f32(fx * baseline) (the product in
 *   float64), and fx, fy, cx, cy, doffs, max_depth each on their own.
 *   den = d + doffs.  A pixel has a depth iff d is finite and den > 0; then Z = fb / den, otherwise Z = +inf (bits
 *   0x7F800000, PFM's "unknown": the convention of the sparse maps).  NaN, +-inf and d = -doffs exactly all give +inf;
 *   -0.0 is an ordinary zero; subnormal d, den and Z are kept, not flushed; Z may overflow to +inf or underflow to 0.
 *   The point of pixel (h, w):  X = (((float)w - cx) * Z) / fx,  Y = (((float)h - cy) * Z) / fy  - sub, mul, div.
 *   A pixel becomes a point iff Z is finite and Z <= max_depth (+inf keeps every finite Z; a Z equal to it is kept).
 * mccnn_depth, one streaming launch: depth[h][w] = Z.  map and depth need 4-byte alignment and must not overlap.
 * mccnn_reproject_points, an ordered stream compaction: points holds the kept pixels in raster order as 16-byte records
 *   (X, Y, Z, the bits of the uint32 h * W + w) - the fourth word lets the host colour a point from the image it has -
 *   and *n_points (one device uint32) their number.  Records at index >= n_points are NOT written.  points: H * W * 16
 *   bytes, 16-byte aligned (MCCNN_E_INVALID otherwise); scratch: mccnn_points_scratch_bytes(H, W) bytes, 16-byte aligned,
 *   private to one call in flight, and every word the call reads of it it has written before on the stream, so calls may
 *   follow each other on one scratch.  H * W <= 2^31 - 1, beyond that MCCNN_E_UNSUPPORTED.
 *   Four launches - block counts, two levels of an exclusive prefix sum, the ranked write - whose number and sizes depend
 *   on H and W alone: no read-back, no allocation, no synchronisation, no atomics, and no wait on another workgroup (a
 *   scan level is a launch): capturable.  A pixel's rank is a sum of counts plus its place in a wave's ballot, so the
 *   order and the bytes are a function of the map and the scalars alone, on every run and every replay.
 * Refused before any HIP call (MCCNN_E_INVALID), naming the argument: null pointers, non-positive sizes, fx, fy or fb that
 *   is not finite and > 0, a non-finite cx, cy or doffs, a NaN max_depth, overlapping buffers; a misaligned or short
 *   scratch is MCCNN_E_SCRATCH.  A refused call writes nothing. */
int mccnn_depth(const float *map, int H, int W, float fb, float doffs, float *depth, mccnn_stream_t stream);
size_t mccnn_points_scratch_bytes(int H, int W);    /* 0 for non-positive sizes and beyond the pixel limit */
int mccnn_reproject_points(const float *map, int H, int W, float fx, float fy, float cx, float cy, float fb, float doffs,
                           float max_depth, float *points /* [H*W][4] */, uint32_t *n_points, void *scratch,
                           size_t scratch_bytes, mccnn_stream_t stream);

/* ---- a10 median_filter (pf:403-421): clipped fh x fw window (odd sizes, fh*fw <= 49), np.median -------------
 * np.median to the bit: NaN in the window gives NaN, and a median of -0.0 is +0.0 (np.mean's sum starts from +0).
 * Other window sizes and H > 65535 (rows go on grid.y): MCCNN_E_UNSUPPORTED. */
int mccnn_median(const float *disp, int H, int W, int fh, int fw, float *out, mccnn_stream_t stream);

/* ---- a11 bilateral_filter (pf:424-470) ----------------------------------------------------------------------
 * table: device [fh][fw] float32 spatial kernel (util.normal evaluated on the host, pf:428-436); thr gates
 * |I(q)-I(p)| < thr.  Sums follow NumPy's pairwise order over the clipped window (pf:463,466): bit-exact, a gated-out
 * tap included (0 * NaN = NaN, as NumPy computes it).  Window sizes and the row limit as for mccnn_median. */
int mccnn_bilateral(const float *image, const float *disp, int H, int W, int fh, int fw, const float *table,
                    float thr, float *out, mccnn_stream_t stream);

/* ---- a0  decode + standardise on the device (match.py:118-125) ---------------------------------------------------
 * From the decoded bytes of a PNG to the standardised float32 image the conv stack reads, bit-identical to
 *     g = util.read_gray(p).astype(np.float32);  (g - np.mean(g, axis=(0,1))) / np.std(g, axis=(0,1))
 * as NumPy 2 evaluates it on the host (reduction buffer of 8192 elements; csrc/ingest.hip states the summation order).
 * image_u8: [H][W][C] uint8, C = 1 (grey), 3 (RGB) or 4 (RGBA, the alpha byte ignored).  Grey of a colour pixel:
 * (r*9797 + g*19234 + b*3737) >> 15, libpng's rgb_to_gray as OpenCV sets it up.  out: [H][W] float32.  float32
 * throughout, un-fused, correctly rounded division and square root; a constant image gives NumPy's 0/0 (NaN).
 * scratch: mccnn_ingest_scratch_bytes(H, W) bytes (chunk sums of BOTH views of a pair: the same size serves the
 * one-image call), 4-byte aligned, private to one call in flight.  Three launches per call, no synchronisation.
 * The _pair form takes both views of a stereo pair (same H, W, C) in the same three launches. */
size_t mccnn_ingest_scratch_bytes(int H, int W); /* 0 for non-positive sizes */
int mccnn_ingest_u8(const uint8_t *image_u8, int H, int W, int C, float *out, void *scratch, size_t scratch_bytes,
                    mccnn_stream_t stream);
int mccnn_ingest_u8_pair(const uint8_t *left_u8, const uint8_t *right_u8, int H, int W, int C, float *out_left,
                         float *out_right, void *scratch, size_t scratch_bytes, mccnn_stream_t stream);

/* ---- training patches cut on the device (datagenerator.py:137-216; the paper's data set augmentation) -------------
 * N sample records -> N patches out[N][ps][ps], gathered from `pool`, a flat float32 buffer that holds n_images
 * standardised images of any sizes, UNPADDED; images[k] gives image k's offset in floats into the pool and its size.
 * A record names its image, the centre (cy, cx) of the patch in it, the row-major 2 x 2 matrix m that maps an offset in
 * the patch (x first) to an offset in the image, and a gain and a bias.  For output pixel (i, j), c = (ps - 1) / 2,
 * u = j - c, v = i - c, float32 throughout, every operation rounded on its own, in this order:
 *     x  = cx + ((m[0]*u) + (m[1]*v))          y  = cy + ((m[2]*u) + (m[3]*v))
 *     x0 = floorf(x), fx = x - x0              y0 = floorf(y), fy = y - y0
 *     tap(yf, xf) = I[(int)yf][(int)xf] if 0 <= yf <= H-1 and 0 <= xf <= W-1 (compared as floats, before any conversion),
 *                   else +0.0f: the reference's zero padding
 *     row(yy) = tap(yy, x0)                                        if fx == 0   (the second tap is not read)
 *             = (tap(yy,x0) * (1 - fx)) + (tap(yy,x0+1) * fx)      otherwise
 *     val     = row(y0)                                            if fy == 0
 *             = (row(y0) * (1 - fy)) + (row(y0+1) * fy)            otherwise
 *     out     = val                                                if gain == 1 and bias == 0
 *             = (val * gain) + bias                                otherwise
 * An identity record (integer centre, m = identity, gain 1, bias 0) is therefore a plain copy, -0.0 pixels included,
 * and a centre far outside the image (+-1e30) reads nothing and yields zeros.
 * records[n].image is TRUSTED (the kernel cannot report an error): the caller checks 0 <= image < n_images before the
 * upload.  One launch, one workgroup per patch in a grid-stride loop, so N is limited by the output's size alone.
 * Refused: null pointers, N < 1, n_images < 1, an even or non-positive ps (MCCNN_E_INVALID); ps > 31
 * (MCCNN_E_UNSUPPORTED). */
typedef struct { int64_t offset; int32_t H, W; } mccnn_sample_image_t;                        /* 16 bytes */
typedef struct { int32_t image; float cy, cx; float m[4]; float gain, bias; } mccnn_sample_t; /* 36 bytes */
int mccnn_sample_patches(const float *pool, const mccnn_sample_image_t *images, int n_images,
                         const mccnn_sample_t *records, int N, int ps, float *out /* [N][ps][ps] */,
                         mccnn_stream_t stream);

/* ---- evaluation of a disparity map against ground truth, on the device (the Middlebury SDK's evaldisp, as remembered) ---
 * Regions.  A pixel belongs to `all` when gt is finite (+inf is Middlebury's "unknown"; NaN and -inf are treated the
 *   same), to `nonocc` when it is also mask == 255 (every other mask value - 0 unknown, 128 occluded, anything else -
 *   excludes it); with mask == NULL nonocc equals all.
 * Per pixel of a region: n_valid += 1.  disp not finite or disp < 0 (the pipeline's -1 for "no winner", any NaN; -0.0f is
 *   valid): n_invalid += 1 and nothing else.  Otherwise err = fabsf(disp - gt), one float32 subtraction; n_bad[k] += 1
 *   when err > thresholds[k] (strict float32 compare); the pixel's terms are a = (double)err and q = (double)err *
 *   (double)err (exact in float64).
 * Sums, defined to the bit.  Pixels are numbered i = h*W + w and cut into chunks of 1024 consecutive indices.  A chunk's
 *   1024 terms (+0.0 for a pixel outside the region, invalid or past the end) are reduced by the stride-halving tree
 *   for s = 512, 256, ..., 1: x[j] += x[j+s] for j < s; the chunk partials are added in ascending chunk order starting
 *   from +0.0.  The same tree serves sum_abs (terms a) and sum_sq (terms q) of both regions.
 * accumulate == 0: result is overwritten, n_bad[k] for k >= n_thr written as 0.  Otherwise the counts are added to what
 *   result holds (n_bad[k], k >= n_thr, left untouched) and each sum becomes old + this call's total, one float64
 *   addition: a list's totals build up on the device with no read-back per pair.
 * thresholds: HOST array of n_thr values, read at call time and passed to the kernel by value.
 * scratch: mccnn_evaluate_scratch_bytes(H, W) bytes (per chunk: four float64 partials and twenty uint32 counts), 8-byte
 *   aligned like result, private to one call in flight.  Two launches, no synchronisation, no atomics: capturable.
 * Refused before any HIP call: null disp / gt / thresholds / result / scratch, non-positive sizes, n_thr outside 1..8, a
 *   NaN threshold, misaligned scratch / result (MCCNN_E_INVALID); scratch_bytes too small (MCCNN_E_SCRATCH); H*W above
 *   1024 * (2^31 - 1), the chunk index being the workgroup index of the first launch (MCCNN_E_UNSUPPORTED). */
#define MCCNN_EVAL_MAX_THRESHOLDS 8
typedef struct { uint64_t n_valid, n_invalid, n_bad[MCCNN_EVAL_MAX_THRESHOLDS]; double sum_abs, sum_sq; } mccnn_eval_region_t; /* 96 bytes */
typedef struct { mccnn_eval_region_t all, nonocc; } mccnn_eval_t;                                                              /* 192 bytes */
size_t mccnn_evaluate_scratch_bytes(int H, int W); /* 0 for non-positive sizes */
int mccnn_evaluate(const float *disp, const float *gt, const uint8_t *mask /* may be NULL */, int H, int W,
                   const float *thresholds /* HOST, n_thr values */, int n_thr, int accumulate,
                   mccnn_eval_t *result /* device */, void *scratch, size_t scratch_bytes, mccnn_stream_t stream);

/* ---- exact error quantiles (Middlebury's A50, A90, A95, A99) of a map, and a list's pooled quantiles, on the device -----
 * Regions, validity and error are those of mccnn_evaluate: `all` is the pixels whose gt is finite, `nonocc` those with
 *   also mask == 255 (mask == NULL: nonocc equals all); an estimate is invalid when it is not finite or < 0 (-0.0f is
 *   valid).  A SCORED pixel of a region is one in the region with a valid estimate.  Its error is err = fabsf(disp - gt):
 *   one float32 subtraction, subnormals kept, +inf when the subtraction overflows; a NaN cannot occur.  Its KEY is the
 *   uint32 bit pattern of err: for non-negative floats the key order is the value order, so "smallest" means smallest key.
 * Quantiles.  A quantile is an integer q_ppm in 1 .. 1 000 000, parts per million: A90 is 900000.  For a region with n
 *   scored pixels the rank is r = max(ceil(q_ppm * n / 10^6) - 1, 0), in exact 64-bit integer arithmetic
 *   (q_ppm * n + 999999) / 1000000 - 1; the value is the key of rank r (0-based) among the region's scored pixels in
 *   ascending order - the nearest-rank quantile, NumPy's method="inverted_cdf".  n == 0: the value is the canonical NaN
 *   0x7fc00000 and the rank 0.  Ties need no rule: equal keys are equal values.  Repeated and unordered q_ppm are allowed.
 * Pool.  A list's pooled quantiles come from a device-resident histogram pool[2][65536] of uint64, region then key >> 16,
 *   which the caller zeroes once and every call that is given it adds its scored pixels to.  The pooled value of a
 *   quantile is the float whose bits are bin << 16 for the bin that holds rank r of the pooled counts, NaN when the pool
 *   is empty.  Truncation to the top 16 bits is monotone, so the pooled value is the top 16 bits of the exact pooled order
 *   statistic: a relative resolution of 2^-7, still defined to the bit.
 * mccnn_evaluate_quantiles.  result != NULL: the pair's exact quantiles overwrite it, entries k >= n_q written as rank 0
 *   and value +0.0f.  pool != NULL: the pair's scored pixels are added to the pool.  Both may be given, with both NULL the
 *   call is refused; the bits of result do not depend on whether pool is given.  q_ppm: HOST array of n_q values, read at
 *   call time and passed to the kernels by value.  scratch: mccnn_evaluate_quantiles_scratch_bytes(H, W) bytes, 8-byte
 *   aligned like result and pool, private to one call in flight; the call clears what it needs of it on the stream, so
 *   calls may follow each other on one scratch.  A four-pass radix selection over the key's bytes: every pass reads disp,
 *   gt and mask again, no error map is stored, the ranks are computed on the device.  Only integer atomics touch memory,
 *   and integer sums commute: the same bits from every call and every replay of a captured graph.  No allocation, no
 *   synchronisation: capturable.
 * mccnn_evaluate_quantiles_pooled: the pooled values of the pool as it stands, n_scored the pool's total; one launch.
 * Refused before any HIP call: null disp / gt / q_ppm / scratch (pooled: pool / q_ppm / result), result and pool both
 *   NULL, non-positive sizes, n_q outside 1..8, a q_ppm outside 1..10^6, misaligned scratch / result / pool
 *   (MCCNN_E_INVALID); scratch_bytes too small (MCCNN_E_SCRATCH); H*W above 2^32 - 1, the reach of the 32-bit bin counts
 *   (MCCNN_E_UNSUPPORTED). */
#define MCCNN_EVAL_MAX_QUANTILES 8
typedef struct { uint64_t n_scored; uint64_t rank[MCCNN_EVAL_MAX_QUANTILES]; float value[MCCNN_EVAL_MAX_QUANTILES]; } mccnn_quantile_region_t; /* 104 bytes */
typedef struct { mccnn_quantile_region_t all, nonocc; } mccnn_eval_quantiles_t;                                                              /* 208 bytes */
#define MCCNN_EVAL_POOL_BYTES (2 * 65536 * 8)
size_t mccnn_evaluate_quantiles_scratch_bytes(int H, int W); /* 0 for non-positive sizes */
int mccnn_evaluate_quantiles(const float *disp, const float *gt, const uint8_t *mask /* may be NULL */, int H, int W,
                             const uint32_t *q_ppm /* HOST, n_q values */, int n_q,
                             mccnn_eval_quantiles_t *result /* device, may be NULL */, uint64_t *pool /* device, may be NULL */,
                             void *scratch, size_t scratch_bytes, mccnn_stream_t stream);
int mccnn_evaluate_quantiles_pooled(const uint64_t *pool, const uint32_t *q_ppm /* HOST */, int n_q,
                                    mccnn_eval_quantiles_t *result /* device */, mccnn_stream_t stream);

/* ---- KITTI 2012 / 2015: the development kit's file code, background interpolation and error rule, on the device ------
 * Written down from memory of the kit; THIS text is the binding definition.  Throughout, a disparity is
 * VALID when it is finite and >= 0: -0.0f is valid; -1, NaN and +-inf are not (the rule of mccnn_evaluate).  Device
 * pointers, sizes and a stream; no allocation, no synchronisation, no atomics: capturable.  Arguments are validated
 * before any HIP call: null pointers, non-positive sizes, misaligned pointers (float32 4, uint16 2, scratch and result 8
 * bytes) are MCCNN_E_INVALID, a scratch too small is MCCNN_E_SCRATCH, H*W beyond the grid's reach MCCNN_E_UNSUPPORTED.
 *
 * (a) mccnn_kitti_encode_u16: the float32 map [H][W] as the kit's 16-bit code [H][W].  An invalid disparity -> 0 ("no
 *   value").  Otherwise v = rintf(disp * 256.0f) - one float32 multiply, round half to even - clamped to 1 .. 65535; the
 *   lower clamp keeps a valid zero disparity from reading back as "no value".  (The kit truncates; rounding halves the
 *   quantisation error and is this project's choice.)  One launch.
 *   mccnn_kitti_decode_u16 is the way back, what a reader of the file sees: code / 256.0f (exact in float32), 0 -> +inf -
 *   Middlebury's "unknown" as a ground truth, an invalid disparity as an estimate.  One launch.
 *
 * (b) mccnn_kitti_interpolate_background (out != disp): the kit's interpolateBackground, stated without its sequential
 *   walk.  Row pass, on disp, for every invalid pixel: L is the nearest valid pixel to its left in its row, R the nearest
 *   valid pixel to its right; with both the value is R < L ? R : L (float32 compare: L on a tie, and for -0.0f against
 *   +0.0f); with one, that one; with neither the pixel keeps its bits.  After the row pass a pixel is invalid only if its
 *   whole row was.  Column pass, on the row pass's result: an invalid pixel above the first valid pixel of its column takes
 *   that pixel's value, one below the last valid pixel takes that one's; an invalid pixel between two valid pixels of its
 *   column (a whole invalid row inside the image) stays as it is, as in the kit, and so does a column without a valid pixel.
 *   Valid pixels are copied bit for bit.  Two launches (one workgroup per row; one thread per column).
 *
 * (c) mccnn_evaluate_kitti writes the mccnn_eval_t of mccnn_evaluate from 16-bit ground truth [H][W].  Region `all`: the
 *   pixels with gt_occ != 0, truth g = gt_occ / 256.0f (exact in float32).  Region `nonocc`: the pixels with gt_noc != 0,
 *   truth from gt_noc; with gt_noc == NULL it equals `all`.  Per pixel of a region: n_valid += 1; an invalid estimate adds
 *   n_invalid += 1 and nothing else; otherwise err = fabsf(d - g), n_bad[k] += 1 when err > abs_thr[k] && err > rel_thr[k]
 *   * g - the product a float32 multiply rounded on its own (no FMA contraction), both compares strict; KITTI 2015's D1 is
 *   (3, 0.05), KITTI 2012's Out-Noc / Out-All at t pixels are (t, 0) - and the pixel's terms a = (double)err, q = a * a go
 *   into sum_abs and sum_sq.  The sums are defined to the bit by the tree of mccnn_evaluate (chunks of 1024 pixel indices,
 *   stride-halving tree, chunk partials added in ascending order from +0.0), and `accumulate` means what it means there.
 *   interpolate != 0: the map scored is (b) applied to disp, held in scratch (two more launches); disp is never written.
 *   abs_thr, rel_thr: HOST arrays of n_thr values each, read at call time.  scratch: mccnn_evaluate_kitti_scratch_bytes(H,
 *   W, interpolate) bytes, 8-byte aligned like result, private to one call in flight.
 *   Refused as well: n_thr outside 1 .. MCCNN_EVAL_MAX_THRESHOLDS, a NaN or negative threshold (MCCNN_E_INVALID). */
int mccnn_kitti_encode_u16(const float *disp, int H, int W, uint16_t *out_u16, mccnn_stream_t stream);
int mccnn_kitti_decode_u16(const uint16_t *code_u16, int H, int W, float *out, mccnn_stream_t stream);
int mccnn_kitti_interpolate_background(const float *disp, int H, int W, float *out, mccnn_stream_t stream);
size_t mccnn_evaluate_kitti_scratch_bytes(int H, int W, int interpolate); /* 0 for non-positive sizes */
int mccnn_evaluate_kitti(const float *disp, const uint16_t *gt_occ_u16, const uint16_t *gt_noc_u16 /* may be NULL */,
                         int H, int W, const float *abs_thr /* HOST */, const float *rel_thr /* HOST */, int n_thr,
                         int interpolate, int accumulate, mccnn_eval_t *result /* device */, void *scratch,
                         size_t scratch_bytes, mccnn_stream_t stream);

/* ---- a1 epilogues of the conv stack (model.py:51-64, 111-125) ------------------------------------------------
 * mccnn_bias_act: x[n][c][i] = act(x[n][c][i] + bias[c]) in place on an NCHW tensor (plane = H*W elements) -
 *   tf.nn.bias_add + tf.nn.relu of model.py:118-123 in ONE pass over the activations (relu != 0), or the bias
 *   alone (relu == 0).  The convolution itself runs in PyTorch-ROCm/MIOpen without bias.  The ReLU here and in
 *   mccnn_conv1_pad_bias_relu keeps a NaN (as NumPy's, torch's and TensorFlow's do) and gives +0.0 for -0.0; N*C <= 65535.
 * mccnn_l2norm_chw_to_hwc: tf.nn.l2_normalize over channels (model.py:64), x * rsqrt(max(sum x^2, 1e-12)), fused
 *   with the last layer's bias (bias may be NULL) and the layout change NCHW [C][H][W] -> NHWC [H][W][C]; a NaN
 *   channel makes its whole pixel NaN (tf.maximum keeps a NaN sum).  C = 64 only (MCCNN_E_UNSUPPORTED otherwise). */
int mccnn_bias_act(float *x, const float *bias, int N, int C, long plane, int relu, mccnn_stream_t stream);
/* First layer fused with the input padding (pf:20-25, model.py:51-53): images [N][H][W] -> out [N][C][H+2pad-2]
 * [W+2pad-2] = relu(conv3x3_valid(zero_pad(image, pad), weights [C][1][3][3]) + bias [C]). */
int mccnn_conv1_pad_bias_relu(const float *images, const float *weights, const float *bias, float *out, int N, int H,
                              int W, int pad, int C, mccnn_stream_t stream);
int mccnn_l2norm_chw_to_hwc(const float *chw, const float *bias, float *hwc, int C, int H, int W,
                            mccnn_stream_t stream);

/* ---- a1 on the matrix cores: split-operand 3x3 convolutions (the default feature path; model.py:51-64) ---------
 * The 64 -> 64 map layers as an implicit GEMM on v_mfma_f32_32x32x16_f16 with every float32 operand carried as two
 * f16 numbers (x * s = hi + lo, 22 significand bits; products hi*hi and hi*lo + lo*hi accumulated in float32 in two
 * accumulator sets that meet once per output): as close to a float64 evaluation as the float32 library convolutions
 * (2.5e-7 .. 3.9e-7 on the unit feature vectors, the library 2.7e-7 .. 3.4e-7, up to 1500 x 1000), not bit-identical
 * to them.
 * saturation_flag (device int, may be NULL): set to 1 when a stored activation exceeds the f16 range of the records
 * (|x| * act_scale > 65504; the value is clamped, the features are then NOT float32-accurate).  Only stored pixels
 * count: what a ragged tile computes beyond the last column or row of the output never sets it.  The caller zeroes
 * it, reads it back after the pair and recomputes with the float32 library path if it is set (match.py does).
 * "Split records": 256 bytes per pixel, [channel group q of 16][hi: 16 x f16 | lo: 16 x f16], pixel-major
 * [N][H][W][256 B]; act_scale (a power of two, e.g. 256) is the factor the stored activations carry (they saturate
 * at |x| * act_scale = 65504).
 * mccnn_conv3x3_split_pack: weights [64][64][3][3] float32 (out, in, ky, kx) -> `packed`
 *   (mccnn_conv3x3_split_weights_bytes() bytes) in MFMA fragment order, scaled by weight_scale (a power of two that
 *   brings max |w| near 1024).
 * mccnn_conv1_split: layer 1 (1 -> 64 maps) fused with the zero padding like mccnn_conv1_pad_bias_relu, writing
 *   split records [N][H+2pad-2][W+2pad-2].
 * mccnn_conv3x3_split: in [N][Hi][Wi] records -> VALID conv + bias; last == 0: ReLU, split records
 *   [N][Hi-2][Wi-2]; last != 0: tf.nn.l2_normalize over the 64 maps, float32 [N][Hi-2][Wi-2][64] (what
 *   mccnn_cost_volume reads). */
size_t mccnn_conv3x3_split_weights_bytes(void);
int mccnn_conv3x3_split_pack(const float *weights, float weight_scale, void *packed, mccnn_stream_t stream);
int mccnn_conv1_split(const float *images, const float *weights, const float *bias, void *out, int N, int H, int W,
                      int pad, float act_scale, int *saturation_flag, mccnn_stream_t stream);
int mccnn_conv3x3_split(const void *in, const void *packed_weights, const float *bias, void *out, int N, int Hi, int Wi,
                        float weight_scale, float act_scale, int last, int *saturation_flag, mccnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCCNN_H */
