"""Device-resident stages of the hot path: thin, allocation-aware wrappers over the C ABI (include/mccnn.h).

Everything here takes and returns torch device tensors; nothing touches host memory and nothing is computed by
PyTorch except the 5-layer conv stack (model.NET).  The NumPy-facing drop-in lives in process_functional.py and the
whole-pair driver (the timed region of the reference's match.py:129-179) is StereoMatcher.match below.
"""
import collections
import ctypes
import math

import numpy as np
import torch

import _hipabi as hip
from calibration import Calibration
from pair_result import PairResult
from semi_dense_rule import SemiDenseRule  # noqa: F401  (host-only: match.py parses it before the GPU is pinned)


def _f32(x):
    """The float32 rounding NumPy 2 applies when a Python scalar meets a float32 array."""
    return float(np.float32(x))


class StageTimer(object):
    """Optional per-stage HIP-event timing on the stream the kernels run on (bench.py turns it on)."""

    def __init__(self, enabled=False):
        self.enabled = enabled
        self.records = []  # (name, start_event, end_event)
        self.spans = []    # [name, start_event, end_event or None while open]
        self._open = None

    def start(self, name):
        if not self.enabled:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._open = (name, ev)

    def stop(self):
        if not self.enabled or self._open is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((self._open[0], self._open[1], ev))
        self._open = None

    def span_start(self, name):
        """A bracket around several launches (a whole stage, possibly on several streams that fork from and join the
        current one): kept apart from the per-launch records."""
        if self.enabled:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.spans.append([name, ev, None])

    def span_stop(self, name):
        if self.enabled:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            for s in reversed(self.spans):
                if s[0] == name and s[2] is None:
                    s[2] = ev
                    break

    def spans_ms(self):
        out = {}
        for name, a, b in self.spans:
            if b is not None:
                out.setdefault(name, []).append(a.elapsed_time(b))
        return out

    def summary_ms(self):
        """{name: [ms, ...]} - call after torch.cuda.synchronize()."""
        out = {}
        for name, a, b in self.records:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return out


_NO_TIMER = StageTimer(False)


# ---- a1 ----------------------------------------------------------------------------------------------------------
def bias_act_(x, bias, relu):
    """In place on a contiguous NCHW tensor: x = relu(x + bias[c]) (or the bias alone) in one pass (model.py:118-123)."""
    N, C, H, W = x.shape
    assert x.is_contiguous() and bias.numel() == C
    hip.check(hip.load().mccnn_bias_act(hip.ptr(x), hip.ptr(bias), N, C, H * W, 1 if relu else 0, hip.stream()),
              "mccnn_bias_act")
    return x


def conv1_pad_bias_relu(images, weight, bias, pad):
    """images [N,H,W] -> [N,C,H+2pad-2,W+2pad-2]: zero padding + first 3x3 VALID conv (1 -> C maps) + bias + ReLU in one
    launch (pf:20-25, model.py:51-53).  weight: torch layout [C,1,3,3]."""
    N, H, W = images.shape
    C = weight.shape[0]
    assert tuple(weight.shape) == (C, 1, 3, 3) and images.is_contiguous() and weight.is_contiguous()
    out = torch.empty((N, C, H + 2 * pad - 2, W + 2 * pad - 2), dtype=torch.float32, device=images.device)
    hip.check(hip.load().mccnn_conv1_pad_bias_relu(hip.ptr(images), hip.ptr(weight), hip.ptr(bias), hip.ptr(out), N, H,
                                                   W, int(pad), C, hip.stream()), "mccnn_conv1_pad_bias_relu")
    return out


def l2norm_chw_to_hwc(chw, bias=None, out=None):
    """[C,H,W] conv output (+ the last layer's bias) -> [H,W,C] unit feature vectors (model.py:64)."""
    C, H, W = chw.shape
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=chw.device)
    assert tuple(out.shape) == (H, W, C) and out.is_contiguous()
    hip.check(hip.load().mccnn_l2norm_chw_to_hwc(hip.ptr(chw), hip.ptr(bias) if bias is not None else None,
                                                 hip.ptr(out), C, H, W, hip.stream()), "mccnn_l2norm_chw_to_hwc")
    return out


# ---- a1 on the matrix cores (opt-in): split-operand convolutions, csrc/conv_mfma.hip ---------------------------------
SPLIT_ACT_SCALE = 256.0   # stored activations carry this factor (power of two); they saturate at |x| = 65504 / 256


def conv3x3_split_pack(weight):
    """weight [64,64,3,3] (torch layout) -> (packed device buffer, weight_scale) for conv3x3_split.  Reads max |w|
    back to the host to choose the power-of-two scale: call once per weight set, not per image."""
    assert tuple(weight.shape) == (64, 64, 3, 3), "the split-operand kernel is built for 64 -> 64 maps, 3x3"
    w = weight.detach().contiguous().float()
    m = float(w.abs().max())
    scale = 2.0 ** math.floor(math.log2(1024.0 / m)) if m > 0.0 and math.isfinite(m) else 1.0
    lib = hip.load()
    packed = torch.empty((lib.mccnn_conv3x3_split_weights_bytes(),), dtype=torch.uint8, device=w.device)
    hip.check(lib.mccnn_conv3x3_split_pack(hip.ptr(w), scale, hip.ptr(packed), hip.stream()), "mccnn_conv3x3_split_pack")
    return packed, scale


def conv1_split(images, weight, bias, pad, act_scale=SPLIT_ACT_SCALE, sat_flag=None):
    """images [N,H,W] -> split records [N,H+2pad-2,W+2pad-2,256] (uint8 view): padding + layer 1 + bias + ReLU.
    sat_flag: int32 device tensor [1] that the kernel sets when an activation leaves the records' f16 range."""
    N, H, W = images.shape
    assert tuple(weight.shape) == (64, 1, 3, 3) and images.is_contiguous() and weight.is_contiguous()
    out = torch.empty((N, H + 2 * pad - 2, W + 2 * pad - 2, 256), dtype=torch.uint8, device=images.device)
    hip.check(hip.load().mccnn_conv1_split(hip.ptr(images), hip.ptr(weight), hip.ptr(bias), hip.ptr(out), N, H, W,
                                           int(pad), float(act_scale), hip.ptr(sat_flag) if sat_flag is not None else None,
                                           hip.stream()), "mccnn_conv1_split")
    return out


def conv3x3_split(x, packed, weight_scale, bias, last, act_scale=SPLIT_ACT_SCALE, sat_flag=None):
    """x: split records [N,Hi,Wi,256] -> VALID 3x3 conv + bias; last=False: ReLU, records [N,Hi-2,Wi-2,256];
    last=True: L2-normalised float32 features [N,Hi-2,Wi-2,64]."""
    N, Hi, Wi, rec = x.shape
    assert rec == 256 and x.dtype == torch.uint8 and x.is_contiguous()
    if last:
        out = torch.empty((N, Hi - 2, Wi - 2, 64), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((N, Hi - 2, Wi - 2, 256), dtype=torch.uint8, device=x.device)
    hip.check(hip.load().mccnn_conv3x3_split(hip.ptr(x), hip.ptr(packed), hip.ptr(bias), hip.ptr(out), N, Hi, Wi,
                                             float(weight_scale), float(act_scale), 1 if last else 0,
                                             hip.ptr(sat_flag) if sat_flag is not None else None, hip.stream()),
              "mccnn_conv3x3_split")
    return out


# ---- a2 ----------------------------------------------------------------------------------------------------------
def cost_volume(fl, fr, ndisp, mode=hip.MCCNN_CV_EXACT, out=None):
    H, W, C = fl.shape
    if out is None:
        lcv = torch.empty((ndisp, H, W), dtype=torch.float32, device=fl.device)
        rcv = torch.empty((ndisp, H, W), dtype=torch.float32, device=fl.device)
    else:
        lcv, rcv = out
    hip.check(hip.load().mccnn_cost_volume(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp), hip.ptr(lcv), hip.ptr(rcv),
                                           int(mode), hip.stream()), "mccnn_cost_volume")
    return lcv, rcv


def cost_volume_hwd(fl, fr, ndisp, out=None, mode=hip.MCCNN_CV_EXACT):
    """cost_volume(mode) written straight into pixel-major volumes [H,W,Dp] (mccnn_cost_volume_hwd)."""
    H, W, C = fl.shape
    dp = hwd_pitch(ndisp)
    if out is None:
        lcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
        rcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
    else:
        lcv, rcv = out
    hip.check(hip.load().mccnn_cost_volume_hwd(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp), hip.ptr(lcv), hip.ptr(rcv),
                                               int(mode), hip.stream()), "mccnn_cost_volume_hwd")
    return lcv, rcv


VERTICAL_RANGE_MAX = 4         # mccnn_cost_volume_vertical_hwd


def cost_volume_vertical_hwd(fl, fr, ndisp, vertical_range, out=None):
    """The bit-exact pixel-major volumes [H,W,Dp] with a vertical search of +-vertical_range rows (0 .. 4) for imperfectly
    rectified pairs (include/mccnn.h: mccnn_cost_volume_vertical_hwd has the definition): each view's pixel keeps, per
    disparity, its best score over the other view's rows h - r .. h + r.  0: the bits of cost_volume_hwd."""
    H, W, C = fl.shape
    dp = hwd_pitch(ndisp)
    if out is None:
        lcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
        rcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
    else:
        lcv, rcv = out
    hip.check(hip.load().mccnn_cost_volume_vertical_hwd(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp), int(vertical_range),
                                                        hip.ptr(lcv), hip.ptr(rcv), hip.stream()),
              "mccnn_cost_volume_vertical_hwd")
    return lcv, rcv


VERTICAL_OFFSET_MAX = 8        # mccnn_vertical_profile, mccnn_cost_volume_offset_hwd
VERTICAL_OFFSET_BLOCK = 64     # pixels per vote block


def vertical_profile_shape(H, W, max_offset, row_step):
    """(n_rows, n_blocks, 2R + 1): the votes array of vertical_profile for an H x W pair."""
    return (int(hip.load().mccnn_vertical_profile_rows(int(H), int(row_step))),
            (int(W) + VERTICAL_OFFSET_BLOCK - 1) // VERTICAL_OFFSET_BLOCK, 2 * int(max_offset) + 1)


def vertical_record(offset, totals):
    """{offset, totals, share} of a measurement on the host: the offset, the votes per candidate -max .. +max and the
    winner's share of all votes (0.0 without votes)."""
    offset = int(np.asarray(offset).reshape(-1)[0])
    totals = [int(t) for t in np.asarray(totals).reshape(-1)]
    n, k = sum(totals), offset + (len(totals) - 1) // 2
    return dict(offset=offset, totals=totals, share=(float(totals[k]) / n if n and 0 <= k < len(totals) else 0.0))


def vertical_profile(fl, fr, ndisp, max_offset, row_step, out=None):
    """The row-offset votes of a pair's features (include/mccnn.h: mccnn_vertical_profile has the definition): int32
    [n_rows, ceil(W / 64), 2 max_offset + 1] holding the uint32 counts, overwritten whatever `out` held."""
    H, W, C = fl.shape
    if not 0 <= int(max_offset) <= VERTICAL_OFFSET_MAX or int(row_step) < 1:       # (the shape below needs them sane)
        raise ValueError("vertical_profile: max_offset=%r outside [0, %d] or row_step=%r < 1"
                         % (max_offset, VERTICAL_OFFSET_MAX, row_step))
    shape = vertical_profile_shape(H, W, max_offset, row_step)
    votes = torch.empty(shape, dtype=torch.int32, device=fl.device) if out is None else out
    hip.check(hip.load().mccnn_vertical_profile(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp), int(max_offset), int(row_step),
                                                hip.ptr(votes), votes.numel() * votes.element_size(), hip.stream()),
              "mccnn_vertical_profile")
    return votes


def vertical_offset_select(votes, max_offset, out=None):
    """(offset int32 [1], totals int64 [2 max_offset + 1]) of a votes array, on the device (mccnn_vertical_offset_select):
    the offset with the most votes, ties to the smaller |k|, then to the negative one; no votes give 0."""
    nk = 2 * int(max_offset) + 1
    if out is None:
        offset = torch.empty((1,), dtype=torch.int32, device=votes.device)
        totals = torch.empty((nk,), dtype=torch.int64, device=votes.device)
    else:
        offset, totals = out
    if votes.dim() != 3 or votes.shape[2] != nk or totals.numel() < nk:
        raise ValueError("vertical_offset_select: votes %s / totals %s do not belong to max_offset=%d"
                         % (tuple(votes.shape), tuple(totals.shape), int(max_offset)))
    hip.check(hip.load().mccnn_vertical_offset_select(hip.ptr(votes), int(votes.shape[0]), int(votes.shape[1]),
                                                      int(max_offset), hip.ptr(offset), hip.ptr(totals), hip.stream()),
              "mccnn_vertical_offset_select")
    return offset, totals


def cost_volume_offset_hwd(fl, fr, ndisp, row_offset, vertical_range, out=None):
    """The bit-exact pixel-major volumes [H,W,Dp] taken along a row offset (include/mccnn.h: mccnn_cost_volume_offset_hwd):
    the search of +-vertical_range rows around row h + k0 of the other view.  row_offset: a device int32 tensor the
    kernel reads k0 from (clamped to +-8), or None for 0 - then the launches of cost_volume_vertical_hwd."""
    H, W, C = fl.shape
    dp = hwd_pitch(ndisp)
    if out is None:
        lcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
        rcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
    else:
        lcv, rcv = out
    if row_offset is not None and (row_offset.dtype != torch.int32 or row_offset.numel() < 1):
        raise ValueError("cost_volume_offset_hwd: row_offset must be a device int32 tensor or None")
    hip.check(hip.load().mccnn_cost_volume_offset_hwd(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp),
                                                      hip.ptr(row_offset) if row_offset is not None else None,
                                                      int(vertical_range), hip.ptr(lcv), hip.ptr(rcv), hip.stream()),
              "mccnn_cost_volume_offset_hwd")
    return lcv, rcv


VERTICAL_FIELD_MAX = 8         # mccnn_vertical_field_select, mccnn_cost_volume_field_hwd: cells either way
VERTICAL_FIELD_MIN_ROWS = 8    # vertical_field_grid: profiled rows a row band keeps at least


def vertical_field_grid(H, W, grid, row_step):
    """The (gh, gw) a requested grid becomes for an H x W pair profiled on every row_step-th row: gw at most the
    ceil(W / 64) vote blocks, gh at most n_rows // 8 so that a row band holds at least 8 profiled rows (cells of a few
    hundred votes select noise), either at least 1."""
    gh, gw = (int(g) for g in grid)
    rows, blocks, _ = vertical_profile_shape(H, W, 0, row_step)
    return max(1, min(gh, rows // VERTICAL_FIELD_MIN_ROWS)), max(1, min(gw, blocks))


def vertical_field_record(offset, totals, field, cell_totals):
    """vertical_record's {offset, totals, share} of the whole image plus the field's: grid [gh, gw], offsets [gh][gw],
    cell_totals [gh][gw][2 max + 1] and cell_shares [gh][gw] (the winner's share of its cell's votes; 0.0 for a cell
    without votes, which holds the global offset)."""
    field = np.asarray(field)
    cells = np.asarray(cell_totals).reshape(field.shape + (-1,))
    record = vertical_record(offset, totals)
    R = (cells.shape[2] - 1) // 2
    shares = []
    for a in range(field.shape[0]):
        shares.append([])
        for b in range(field.shape[1]):
            n, k = int(cells[a, b].sum()), int(field[a, b]) + R
            shares[a].append(float(int(cells[a, b, k])) / n if n and 0 <= k < cells.shape[2] else 0.0)
    record.update(grid=[int(field.shape[0]), int(field.shape[1])], offsets=[[int(v) for v in row] for row in field],
                  cell_totals=[[[int(v) for v in cell] for cell in row] for row in cells], cell_shares=shares)
    return record


def vertical_field_select(votes, H, row_step, max_offset, grid, out=None):
    """(field int32 [gh, gw], cell totals int64 [gh, gw, 2 max_offset + 1], offset int32 [1], totals int64 [2 max_offset
    + 1]) of the votes vertical_profile wrote for an image of H rows at this row_step, on the device
    (mccnn_vertical_field_select): per cell of the grid the offset with the most votes, by vertical_offset_select's rule;
    a cell without votes takes the whole image's, which with its totals is what vertical_offset_select returns."""
    nk = 2 * int(max_offset) + 1
    gh, gw = (int(g) for g in grid)
    if out is None:
        if not (1 <= gh <= VERTICAL_FIELD_MAX and 1 <= gw <= VERTICAL_FIELD_MAX):      # (the shapes below need them sane)
            raise ValueError("vertical_field_select: grid %dx%d outside [1, %d]" % (gh, gw, VERTICAL_FIELD_MAX))
        field = torch.empty((gh, gw), dtype=torch.int32, device=votes.device)
        cells = torch.empty((gh, gw, nk), dtype=torch.int64, device=votes.device)
        offset = torch.empty((1,), dtype=torch.int32, device=votes.device)
        totals = torch.empty((nk,), dtype=torch.int64, device=votes.device)
    else:
        field, cells, offset, totals = out
    if votes.dim() != 3 or votes.shape[2] != nk or totals.numel() < nk or field.numel() < gh * gw \
            or cells.numel() < gh * gw * nk:
        raise ValueError("vertical_field_select: votes %s / field %s / totals %s, %s do not belong to max_offset=%d and a "
                         "%dx%d grid" % (tuple(votes.shape), tuple(field.shape), tuple(cells.shape), tuple(totals.shape),
                                         int(max_offset), gh, gw))
    hip.check(hip.load().mccnn_vertical_field_select(hip.ptr(votes) if votes.numel() else None, int(votes.shape[0]),
                                                     int(votes.shape[1]), int(H), int(row_step), int(max_offset), gh, gw,
                                                     hip.ptr(field), hip.ptr(cells), hip.ptr(offset), hip.ptr(totals),
                                                     hip.stream()),
              "mccnn_vertical_field_select")
    return field, cells, offset, totals


def cost_volume_field_hwd(fl, fr, ndisp, field, vertical_range, out=None):
    """The bit-exact pixel-major volumes [H,W,Dp] taken along a field of row offsets (include/mccnn.h:
    mccnn_cost_volume_field_hwd): field is a device int32 tensor [gh, gw] the kernel reads (every word clamped to +-8); a
    left pixel takes the word of its own cell, a right pixel that of its row band and of its left partner's column."""
    H, W, C = fl.shape
    dp = hwd_pitch(ndisp)
    if out is None:
        lcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
        rcv = torch.zeros((H, W, dp), dtype=torch.float32, device=fl.device)
    else:
        lcv, rcv = out
    if field is None or field.dtype != torch.int32 or field.dim() != 2 or not field.is_contiguous():
        raise ValueError("cost_volume_field_hwd: field must be a contiguous device int32 tensor [gh, gw]")
    hip.check(hip.load().mccnn_cost_volume_field_hwd(hip.ptr(fl), hip.ptr(fr), H, W, C, int(ndisp), hip.ptr(field),
                                                     int(field.shape[0]), int(field.shape[1]), int(vertical_range),
                                                     hip.ptr(lcv), hip.ptr(rcv), hip.stream()),
              "mccnn_cost_volume_field_hwd")
    return lcv, rcv


# ---- a2 for the accurate network: the decision MLP per (pixel, disparity) ------------------------------------------
DECISION_UNITS = 384                     # csrc/decision_mfma.hip
DECISION_MAPS = (64, 112)
DECISION_FC_LAYERS = (3, 4)
DECISION_MAX_D = 1024
DECISION_LIBRARY_BYTES = 256 << 20       # library route: bytes one [voxels, units] float32 intermediate may take


def decision_kernel_refusal(net, W, D):
    """None when csrc/decision_mfma.hip serves this network and shape, else the limit it exceeds (a sentence)."""
    if net.num_conv_feature_maps not in DECISION_MAPS:
        return "%d feature maps (the decision kernel serves %s)" % (net.num_conv_feature_maps, " or ".join(
            str(c) for c in DECISION_MAPS))
    if net.num_fc_units != DECISION_UNITS:
        return "%d units per hidden layer (the decision kernel is built for %d)" % (net.num_fc_units, DECISION_UNITS)
    if net.num_fc_layers not in DECISION_FC_LAYERS:
        return "%d fully-connected layers (the decision kernel serves 3 or 4)" % net.num_fc_layers
    if D < 2 or D > DECISION_MAX_D:
        return "ndisp=%d outside [2, %d]" % (D, DECISION_MAX_D)
    if D > W - 2:
        return "ndisp=%d needs an image at least ndisp + 2 pixels wide (W=%d)" % (D, W)
    return None


DECISION_SCALE_MAX_EXP = 118            # scale <= 2^118: scale * 256 = 2^126 and 1 / (scale * 256) are normal float32
DECISION_SCALE_MIN_EXP = -126
DECISION_EQUALISE_MAX_EXP = 64          # |log2 c_k| <= 64: c_k * bias and w / c_k stay far from float32's ends


def decision_weight_scale(m):
    """The power of two the decision kernel's weights are packed with, from m = max |w| over the packed layers (pure:
    no device).  scale = 2^e, e = floor(log2(1024 / m)), i.e. m * scale in (512, 1024] - the f16 operands then end at
    1024 of 65504 and a hi + lo pair keeps 22 bits down to |w * scale| = 0.25 - and e clamped to [DECISION_SCALE_MIN_EXP,
    DECISION_SCALE_MAX_EXP], so that scale, scale * 256 (the activations' factor) and the reciprocal the kernel
    multiplies by are finite, normal float32 numbers whatever m is.  Weights below 2^-24 / scale then become 0: with
    the clamp active that is |w| < 2^-142, nothing a float32 sum can see.  m = 0 (all-zero weights): 1.  A negative,
    infinite or NaN m is refused: such weights have no packed form, and scale 1 with a clamp to +-65504 - the earlier
    rule - returned finite scores where the network's are inf or NaN."""
    m = float(m)
    if not (math.isfinite(m) and m >= 0.0):
        raise ValueError("decision_weight_scale: max |w| = %r, the decision kernel packs finite weights only" % m)
    if m == 0.0:
        return 1.0
    f, x = math.frexp(m)                   # m = f * 2^x, f in [0.5, 1): 1024 / m = (1 / f) * 2^(10 - x), 1 / f in (1, 2]
    e = 10 - x + (1 if f == 0.5 else 0)    # floor(log2(1024 / m)) without log2's rounding
    return 2.0 ** max(DECISION_SCALE_MIN_EXP, min(DECISION_SCALE_MAX_EXP, e))


def decision_equalise_exponents(maxima):
    """maxima: max |w| of each hidden layer the decision kernel packs (fc 2 .. n_fc) -> [log2 c_k], the exact
    power-of-two factors that bring every layer's largest weight into ONE binade, so that the single weight_scale of
    the packed operands serves each of them with all 22 bits:
        W'_k = W_k * c_k / c_(k-1),  b'_k = b_k * c_k  (c_1 = 1),  w_final' = w_final / c_n.
    relu(c x) = c relu(x) for c > 0, so the network function is unchanged; in float32 the products are exact (powers
    of two) short of overflow and underflow.  The common binade is the mean of the layers' own (rounded): the product
    of the layer gains is kept, each layer gets an equal share, and log2 c_n stays within half the number of layers, so
    the last hidden layer and w_final keep their magnitude.  Layers whose largest weights already share a binade
    (glorot) get c_k = 1 and the same bits as before.  All-zero layers are left alone; |log2 c_k| is clamped to
    DECISION_EQUALISE_MAX_EXP (the equalisation is then partial, and still exact).  Pure: no device."""
    for k, m in enumerate(maxima):
        if not (math.isfinite(float(m)) and float(m) >= 0.0):
            raise ValueError("fc%d: max |w| = %r, the decision kernel packs finite weights only" % (k + 2, float(m)))
    exps = [math.frexp(float(m))[1] if float(m) > 0.0 else None for m in maxima]
    live = [e for e in exps if e is not None]
    if not live:
        return [0] * len(exps)
    target = int(math.floor(sum(live) / float(len(live)) + 0.5))
    out, c = [], 0
    for e in exps:
        if e is not None:
            c = max(-DECISION_EQUALISE_MAX_EXP, min(DECISION_EQUALISE_MAX_EXP, c + target - e))
        out.append(c)
    return out


def decision_pack(weights, n_fc, mode):
    """weights [n_fc-1, units, units] (torch layout [out,in]) of the hidden layers 2 .. n_fc -> (packed device buffer,
    weight_scale) for mccnn_cost_volume_accurate*(mode).  Reads max |w| back to the host: once per weight set.  ONE
    scale serves all layers (decision_weight_scale): layers of different magnitude are equalised first
    (ACCURATE_NET.decision_layers).  Non-finite weights are refused."""
    lib = hip.load()
    w = weights.detach().contiguous().float()
    units = int(w.shape[-1])
    nbytes = int(lib.mccnn_decision_pack_bytes(int(n_fc), units, int(mode)))
    if nbytes == 0 or tuple(w.shape) != (n_fc - 1, units, units):
        raise hip.MccnnHipError("mccnn_decision_pack: %d fc layers of %d units are outside the decision kernel's "
                                "envelope (3 or 4 layers of %d units)" % (n_fc, units, DECISION_UNITS))
    try:
        scale = decision_weight_scale(float(w.abs().max()))      # (max propagates NaN)
    except ValueError as e:
        raise hip.MccnnHipError("mccnn_decision_pack: %s" % e)
    packed = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    hip.check(lib.mccnn_decision_pack(hip.ptr(w), int(n_fc), units, scale, int(mode), hip.ptr(packed), hip.stream()),
              "mccnn_decision_pack")
    return packed, scale


def cost_volume_fill(lcv, rcv, ndisp, pixel_major):
    """The border recurrences (pf:94-95, 105-106) on volumes whose w >= d entries are written, in place."""
    H, W = (lcv.shape[0], lcv.shape[1]) if pixel_major else (lcv.shape[1], lcv.shape[2])
    hip.check(hip.load().mccnn_cost_volume_fill(hip.ptr(lcv), hip.ptr(rcv), int(ndisp), H, W, 1 if pixel_major else 0,
                                                hip.stream()), "mccnn_cost_volume_fill")
    return lcv, rcv


def accurate_scores_library(net, aL, aR, ndisp, lcv, rcv, pixel_major, budget=DECISION_LIBRARY_BYTES):
    """The decision network by torch matmuls, float32, on any device: writes -s(h,w,d) to lcv at (h,w,d) and rcv at
    (h,w-d,d) for every w >= d (the other entries are left alone).  Disparity by disparity, in bands of image rows
    sized so that one [voxels, units] intermediate stays under `budget` bytes."""
    H, W, U = aL.shape
    ws = [w.detach() for w in net.fc_weights]
    bs = [b.detach() for b in net.fc_biases]
    lv = lcv.permute(2, 0, 1) if pixel_major else lcv     # [d, h, w] views
    rv = rcv.permute(2, 0, 1) if pixel_major else rcv
    for d in range(int(ndisp)):
        n = W - d
        rows = max(1, min(H, int(budget) // (n * U * 4)))
        for h0 in range(0, H, rows):
            h1 = min(H, h0 + rows)
            x = torch.relu(aL[h0:h1, d:, :] + aR[h0:h1, :n, :]).reshape(-1, U)
            for k in range(1, net.num_fc_layers):
                x = torch.relu(torch.addmm(bs[k], x, ws[k].t()))
            z = torch.addmv(bs[-1].expand(x.shape[0]), x, ws[-1].reshape(-1))
            s = torch.sigmoid(z).neg_().reshape(h1 - h0, n)
            lv[d, h0:h1, d:] = s
            rv[d, h0:h1, :n] = s
    return lcv, rcv


def cost_volume_accurate(net, fl, fr, ndisp, mode=hip.MCCNN_CV_EXACT, decision="kernel", pixel_major=True, out=None,
                         halves=None, sat_flag=None, budget=DECISION_LIBRARY_BYTES):
    """Both cost volumes of the accurate network from the tower outputs fl, fr [H,W,C]: lcv = -s at (h,w,d) for w >= d,
    rcv = -s at (h,w-d,d), border columns by the fast network's recurrences (the same fill launch).
    decision "kernel": csrc/decision_mfma.hip - mode MCCNN_CV_EXACT split operands (float32-accurate), MCCNN_CV_MFMA
    plain f16; sat_flag as for conv3x3_split.  "library": torch matmuls in float32 (accurate_scores_library).
    pixel_major: [H,W,Dp] volumes (else [D,H,W]); out: the two volumes; halves: the two [H,W,units] buffers of the
    first layer's halves (allocated when None)."""
    if decision not in ("kernel", "library"):
        raise ValueError("decision must be 'kernel' or 'library'")
    H, W, C = fl.shape
    D = int(ndisp)
    if out is None:
        shape = (H, W, hwd_pitch(D)) if pixel_major else (D, H, W)
        out = (torch.zeros(shape, dtype=torch.float32, device=fl.device),
               torch.zeros(shape, dtype=torch.float32, device=fl.device))
    lcv, rcv = out
    why = decision_kernel_refusal(net, W, D) if decision == "kernel" else None
    if why is not None:                       # before anything is launched
        raise hip.MccnnHipError("cost_volume_accurate: %s" % why)
    aL, aR = net.first_layer_halves(fl, fr, out=halves)
    if decision == "library":
        accurate_scores_library(net, aL, aR, D, lcv, rcv, pixel_major, budget)
        return cost_volume_fill(lcv, rcv, D, pixel_major)
    lib = hip.load()
    packed, scale, biases, w_final, b_final = net.decision_operands(mode)
    fn = lib.mccnn_cost_volume_accurate_hwd if pixel_major else lib.mccnn_cost_volume_accurate
    hip.check(fn(hip.ptr(aL), hip.ptr(aR), H, W, C, net.num_fc_units, net.num_fc_layers, D, hip.ptr(packed),
                 hip.ptr(biases), hip.ptr(w_final), b_final, scale, hip.ptr(lcv), hip.ptr(rcv), int(mode),
                 hip.ptr(sat_flag) if sat_flag is not None else None, hip.stream()),
              "mccnn_cost_volume_accurate_hwd" if pixel_major else "mccnn_cost_volume_accurate")
    return lcv, rcv


# ---- a0 ----------------------------------------------------------------------------------------------------------
def ingest_scratch(H, W, device):
    """Scratch of one ingest call in flight (the chunk sums of both views): mccnn_ingest_scratch_bytes(H, W) bytes."""
    nbytes = int(hip.load().mccnn_ingest_scratch_bytes(H, W))
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=device)


def _u8_image(image_u8):
    if image_u8.dtype != torch.uint8 or image_u8.dim() not in (2, 3):
        raise ValueError("ingest: expected a uint8 image [H,W] or [H,W,C], got %s %s" % (image_u8.dtype, tuple(image_u8.shape)))
    return image_u8.shape[0], image_u8.shape[1], (image_u8.shape[2] if image_u8.dim() == 3 else 1)


def ingest_u8(image_u8, out=None, scratch=None):
    """uint8 device image [H,W] (grey) or [H,W,C], C = 1, 3 (RGB) or 4 (RGBA, alpha ignored) -> the standardised float32
    image [H,W] match() reads: bit for bit what match.py computes on the host, util.read_gray's grey conversion and
    NumPy's (g - mean) / std in NumPy's summation order (csrc/ingest.hip).  `scratch`: an ingest_scratch()."""
    H, W, C = _u8_image(image_u8)
    out = out if out is not None else torch.empty((H, W), dtype=torch.float32, device=image_u8.device)
    scratch = scratch if scratch is not None else ingest_scratch(H, W, image_u8.device)
    hip.check(hip.load().mccnn_ingest_u8(hip.ptr(image_u8), H, W, C, hip.ptr(out), hip.ptr(scratch),
                                         scratch.numel() * 4, hip.stream()), "mccnn_ingest_u8")
    return out


def ingest_u8_pair(left_u8, right_u8, out_l=None, out_r=None, scratch=None):
    """ingest_u8() on both views of a pair (same shape and channel count) in one call; returns (left, right)."""
    H, W, C = _u8_image(left_u8)
    if _u8_image(right_u8) != (H, W, C):
        raise ValueError("ingest_u8_pair: the two images must have the same shape")
    out_l = out_l if out_l is not None else torch.empty((H, W), dtype=torch.float32, device=left_u8.device)
    out_r = out_r if out_r is not None else torch.empty((H, W), dtype=torch.float32, device=left_u8.device)
    scratch = scratch if scratch is not None else ingest_scratch(H, W, left_u8.device)
    hip.check(hip.load().mccnn_ingest_u8_pair(hip.ptr(left_u8), hip.ptr(right_u8), H, W, C, hip.ptr(out_l), hip.ptr(out_r),
                                              hip.ptr(scratch), scratch.numel() * 4, hip.stream()),
              "mccnn_ingest_u8_pair")
    return out_l, out_r


# ---- evaluation against ground truth ---------------------------------------------------------------------------------
EVAL_BYTES = 192             # sizeof(mccnn_eval_t)
EVAL_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def evaluate_scratch(H, W, device):
    """Scratch of one evaluate() in flight (per-chunk partials and counts): mccnn_evaluate_scratch_bytes(H, W) bytes."""
    nbytes = int(hip.load().mccnn_evaluate_scratch_bytes(H, W))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def evaluate_result(device):
    """A zeroed mccnn_eval_t on the device: 192 bytes as 24 int64 words (an accumulator starts here)."""
    return torch.zeros((EVAL_BYTES // 8,), dtype=torch.int64, device=device)


def evaluate(disp, gt, mask=None, thresholds=EVAL_THRESHOLDS, out=None, accumulate=False, scratch=None):
    """disp, gt: float32 device maps [H,W]; mask: uint8 [H,W] or None (255 = non-occluded) -> the 192-byte device tensor
    (24 int64 words) holding mccnn_eval_t: counts and error sums of the regions `all` (gt finite) and `nonocc` (also mask
    == 255), defined to the bit in include/mccnn.h.  accumulate: add into `out` (which is then required) instead of
    overwriting it.  The thresholds are read here, on the host, at call time - inside a captured graph they and
    `accumulate` are baked in.  No synchronisation; evaluation.Metrics.from_result reads the bytes once they are on the
    host.  `scratch`: an evaluate_scratch()."""
    if disp.dim() != 2 or disp.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError("evaluate: expected float32 maps [H,W], got %s %s and %s %s"
                         % (disp.dtype, tuple(disp.shape), gt.dtype, tuple(gt.shape)))
    if tuple(gt.shape) != tuple(disp.shape):
        raise ValueError("evaluate: the map is %s, the ground truth %s" % (tuple(disp.shape), tuple(gt.shape)))
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(disp.shape)):
        raise ValueError("evaluate: expected a uint8 mask %s, got %s %s" % (tuple(disp.shape), mask.dtype, tuple(mask.shape)))
    for t in (gt, mask, out, scratch):
        if t is not None and t.device != disp.device:
            raise ValueError("evaluate: every tensor must live on the map's device")
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= hip.MCCNN_EVAL_MAX_THRESHOLDS:
        raise ValueError("evaluate: %d thresholds, expected 1..%d" % (len(thr), hip.MCCNN_EVAL_MAX_THRESHOLDS))
    H, W = disp.shape
    if out is None:
        if accumulate:
            raise ValueError("evaluate: accumulate needs the `out` to accumulate into")
        out = torch.empty((EVAL_BYTES // 8,), dtype=torch.int64, device=disp.device)
    elif out.numel() * out.element_size() != EVAL_BYTES:
        raise ValueError("evaluate: `out` must hold %d bytes" % EVAL_BYTES)
    scratch = scratch if scratch is not None else evaluate_scratch(H, W, disp.device)
    hip.check(hip.load().mccnn_evaluate(hip.ptr(disp), hip.ptr(gt), hip.ptr(mask) if mask is not None else None, H, W,
                                        (ctypes.c_float * len(thr))(*thr), len(thr), 1 if accumulate else 0, hip.ptr(out),
                                        hip.ptr(scratch), scratch.numel() * scratch.element_size(), hip.stream()),
              "mccnn_evaluate")
    return out


# ---- exact error quantiles and a list's pooled quantiles (csrc/evaluate_quantiles.hip) --------------------------------
EVAL_QUANTILES_BYTES = 208   # sizeof(mccnn_eval_quantiles_t)
EVAL_QUANTILES_PPM = (500000, 900000, 950000, 990000)    # A50, A90, A95, A99


def evaluate_quantiles_scratch(H, W, device):
    """Scratch of one evaluate_quantiles() in flight (the selection's histograms and state):
    mccnn_evaluate_quantiles_scratch_bytes(H, W) bytes."""
    nbytes = int(hip.load().mccnn_evaluate_quantiles_scratch_bytes(H, W))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)


def evaluate_quantiles_result(device):
    """A zeroed mccnn_eval_quantiles_t on the device: 208 bytes as 26 int64 words."""
    return torch.zeros((EVAL_QUANTILES_BYTES // 8,), dtype=torch.int64, device=device)


def evaluate_quantiles_pool(device):
    """A zeroed pool on the device: the uint64 counts [2][65536] (region, key >> 16) as int64 words; a list's pooled
    quantiles start here."""
    return torch.zeros((2, 65536), dtype=torch.int64, device=device)


def _quantiles_ppm(quantiles_ppm, who):
    ppm = [int(q) for q in quantiles_ppm]
    if not 1 <= len(ppm) <= hip.MCCNN_EVAL_MAX_QUANTILES:
        raise ValueError("%s: %d quantiles, expected 1..%d" % (who, len(ppm), hip.MCCNN_EVAL_MAX_QUANTILES))
    if any(not 1 <= q <= 1000000 for q in ppm):
        raise ValueError("%s: quantiles are parts per million, 1..1000000, got %r" % (who, ppm))
    return (ctypes.c_uint32 * len(ppm))(*ppm), len(ppm)


def _quantiles_pool(pool, device, who):
    if pool.dtype != torch.int64 or pool.numel() * 8 != hip.MCCNN_EVAL_POOL_BYTES or pool.device != device:
        raise ValueError("%s: `pool` must be an evaluate_quantiles_pool() on the map's device" % who)


def evaluate_quantiles(disp, gt, mask=None, quantiles_ppm=EVAL_QUANTILES_PPM, out=None, pool=None, scratch=None):
    """disp, gt: float32 device maps [H,W]; mask: uint8 [H,W] or None (255 = non-occluded) -> the 208-byte device tensor
    (26 int64 words) holding mccnn_eval_quantiles_t: per region n_scored, and for every quantile its rank and the exact
    nearest-rank value of fabsf(disp - gt) over the scored pixels, defined to the bit in include/mccnn.h.  pool: an
    evaluate_quantiles_pool() the map's scored pixels are added to.  out=False: only that - the pool-only call - and None
    is returned.  The quantiles (parts per million) are read here, on the host, at call time - inside a captured graph
    they are baked in.  No synchronisation; evaluation.quantile_raw reads the bytes once they are on the
    host.  `scratch`: an evaluate_quantiles_scratch()."""
    if disp.dim() != 2 or disp.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError("evaluate_quantiles: expected float32 maps [H,W], got %s %s and %s %s"
                         % (disp.dtype, tuple(disp.shape), gt.dtype, tuple(gt.shape)))
    if tuple(gt.shape) != tuple(disp.shape):
        raise ValueError("evaluate_quantiles: the map is %s, the ground truth %s" % (tuple(disp.shape), tuple(gt.shape)))
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(disp.shape)):
        raise ValueError("evaluate_quantiles: expected a uint8 mask %s, got %s %s"
                         % (tuple(disp.shape), mask.dtype, tuple(mask.shape)))
    pool_only = out is False
    for t in (gt, mask, None if pool_only else out, pool, scratch):
        if t is not None and t.device != disp.device:
            raise ValueError("evaluate_quantiles: every tensor must live on the map's device")
    q, n_q = _quantiles_ppm(quantiles_ppm, "evaluate_quantiles")
    H, W = disp.shape
    if pool_only:
        if pool is None:
            raise ValueError("evaluate_quantiles: out=False needs the `pool` to add to")
        out = None
    elif out is None:
        out = torch.empty((EVAL_QUANTILES_BYTES // 8,), dtype=torch.int64, device=disp.device)
    elif out.numel() * out.element_size() != EVAL_QUANTILES_BYTES:
        raise ValueError("evaluate_quantiles: `out` must hold %d bytes" % EVAL_QUANTILES_BYTES)
    if pool is not None:
        _quantiles_pool(pool, disp.device, "evaluate_quantiles")
    scratch = scratch if scratch is not None else evaluate_quantiles_scratch(H, W, disp.device)
    hip.check(hip.load().mccnn_evaluate_quantiles(hip.ptr(disp), hip.ptr(gt), hip.ptr(mask) if mask is not None else None,
                                                  H, W, q, n_q, hip.ptr(out) if out is not None else None,
                                                  hip.ptr(pool) if pool is not None else None, hip.ptr(scratch),
                                                  scratch.numel() * scratch.element_size(), hip.stream()),
              "mccnn_evaluate_quantiles")
    return out


def evaluate_quantiles_pooled(pool, quantiles_ppm=EVAL_QUANTILES_PPM, out=None):
    """pool: an evaluate_quantiles_pool() -> the 208-byte device tensor of evaluate_quantiles() with the pooled values of
    the pool as it stands: the top 16 bits of the exact pooled order statistics (include/mccnn.h).  One launch, no
    synchronisation."""
    _quantiles_pool(pool, pool.device, "evaluate_quantiles_pooled")
    q, n_q = _quantiles_ppm(quantiles_ppm, "evaluate_quantiles_pooled")
    if out is None:
        out = torch.empty((EVAL_QUANTILES_BYTES // 8,), dtype=torch.int64, device=pool.device)
    elif out.numel() * out.element_size() != EVAL_QUANTILES_BYTES or out.device != pool.device:
        raise ValueError("evaluate_quantiles_pooled: `out` must hold %d bytes on the pool's device" % EVAL_QUANTILES_BYTES)
    hip.check(hip.load().mccnn_evaluate_quantiles_pooled(hip.ptr(pool), q, n_q, hip.ptr(out), hip.stream()),
              "mccnn_evaluate_quantiles_pooled")
    return out


# ---- KITTI: the kit's 16-bit code, background interpolation and error rule (csrc/kitti.hip) ---------------------------
def _kitti_map(disp, who):
    if disp.dim() != 2 or disp.dtype != torch.float32:
        raise ValueError("%s: expected a float32 map [H,W], got %s %s" % (who, disp.dtype, tuple(disp.shape)))
    return int(disp.shape[0]), int(disp.shape[1])


def kitti_encode_u16(disp, out=None):
    """disp: float32 device map [H,W] -> uint16 [H,W], the development kit's code: 0 for a pixel without a disparity (not
    finite or < 0), else rint(disp * 256) clamped to 1 .. 65535 (include/mccnn.h).  One launch, no synchronisation."""
    H, W = _kitti_map(disp, "kitti_encode_u16")
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint16, device=disp.device)
    elif out.dtype != torch.uint16 or tuple(out.shape) != (H, W) or out.device != disp.device:
        raise ValueError("kitti_encode_u16: `out` must be a uint16 %s on the map's device" % ((H, W),))
    hip.check(hip.load().mccnn_kitti_encode_u16(hip.ptr(disp), H, W, hip.ptr(out), hip.stream()), "mccnn_kitti_encode_u16")
    return out


def kitti_decode_u16(code, out=None):
    """code: uint16 device plane [H,W] -> float32 [H,W], what a reader of the 16-bit file sees: code / 256, 0 -> +inf
    ("unknown" as a ground truth, no disparity as an estimate).  One launch, no synchronisation."""
    if code.dim() != 2 or code.dtype != torch.uint16:
        raise ValueError("kitti_decode_u16: expected a uint16 plane [H,W], got %s %s" % (code.dtype, tuple(code.shape)))
    H, W = int(code.shape[0]), int(code.shape[1])
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=code.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (H, W) or out.device != code.device:
        raise ValueError("kitti_decode_u16: `out` must be a float32 %s on the plane's device" % ((H, W),))
    hip.check(hip.load().mccnn_kitti_decode_u16(hip.ptr(code), H, W, hip.ptr(out), hip.stream()), "mccnn_kitti_decode_u16")
    return out


def kitti_interpolate_background(disp, out=None):
    """The kit's interpolateBackground (include/mccnn.h): every pixel without a disparity filled from its row - the smaller
    of the nearest valid neighbours - then from its column above the first and below the last valid row.  `out` must not
    be `disp`.  Two launches, no synchronisation."""
    H, W = _kitti_map(disp, "kitti_interpolate_background")
    if out is None:
        out = torch.empty_like(disp)
    elif out.dtype != torch.float32 or tuple(out.shape) != (H, W) or out.device != disp.device:
        raise ValueError("kitti_interpolate_background: `out` must be a float32 %s on the map's device" % ((H, W),))
    hip.check(hip.load().mccnn_kitti_interpolate_background(hip.ptr(disp), H, W, hip.ptr(out), hip.stream()),
              "mccnn_kitti_interpolate_background")
    return out


def evaluate_kitti_scratch(H, W, device, interpolate=False):
    """Scratch of one evaluate_kitti() in flight: mccnn_evaluate_kitti_scratch_bytes(H, W, interpolate) bytes."""
    nbytes = int(hip.load().mccnn_evaluate_kitti_scratch_bytes(H, W, 1 if interpolate else 0))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


KITTI_D1 = ((3.0, 0.05),)    # KITTI 2015: off by more than 3 px and by more than 5 % of the true disparity


def evaluate_kitti(disp, gt_occ, gt_noc=None, thresholds=KITTI_D1, interpolate=False, out=None, accumulate=False,
                   scratch=None):
    """disp: float32 device map [H,W]; gt_occ, gt_noc (or None): uint16 [H,W] as the kit stores them (0 = no ground truth,
    else disparity * 256) -> the 192-byte device tensor of evaluate(): region `all` from gt_occ, `nonocc` from gt_noc.
    thresholds: 1 to 8 (abs, rel) pairs: a pixel is bad when its error exceeds abs pixels and rel times the true disparity.
    interpolate: score kitti_interpolate_background(disp), held in `scratch` (an evaluate_kitti_scratch with the same
    flag).  Everything else as evaluate()."""
    H, W = _kitti_map(disp, "evaluate_kitti")
    for name, t in (("gt_occ", gt_occ), ("gt_noc", gt_noc)):
        if t is not None and (t.dtype != torch.uint16 or tuple(t.shape) != (H, W)):
            raise ValueError("evaluate_kitti: expected a uint16 %s %s, got %s %s" % (name, (H, W), t.dtype, tuple(t.shape)))
    for t in (gt_occ, gt_noc, out, scratch):
        if t is not None and t.device != disp.device:
            raise ValueError("evaluate_kitti: every tensor must live on the map's device")
    pairs = [(float(a), float(r)) for a, r in thresholds]
    if not 1 <= len(pairs) <= hip.MCCNN_EVAL_MAX_THRESHOLDS:
        raise ValueError("evaluate_kitti: %d thresholds, expected 1..%d" % (len(pairs), hip.MCCNN_EVAL_MAX_THRESHOLDS))
    if out is None:
        if accumulate:
            raise ValueError("evaluate_kitti: accumulate needs the `out` to accumulate into")
        out = torch.empty((EVAL_BYTES // 8,), dtype=torch.int64, device=disp.device)
    elif out.numel() * out.element_size() != EVAL_BYTES:
        raise ValueError("evaluate_kitti: `out` must hold %d bytes" % EVAL_BYTES)
    scratch = scratch if scratch is not None else evaluate_kitti_scratch(H, W, disp.device, interpolate)
    floats = ctypes.c_float * len(pairs)
    hip.check(hip.load().mccnn_evaluate_kitti(hip.ptr(disp), hip.ptr(gt_occ), hip.ptr(gt_noc) if gt_noc is not None else None,
                                              H, W, floats(*[a for a, _ in pairs]), floats(*[r for _, r in pairs]),
                                              len(pairs), 1 if interpolate else 0, 1 if accumulate else 0, hip.ptr(out),
                                              hip.ptr(scratch), scratch.numel() * scratch.element_size(), hip.stream()),
              "mccnn_evaluate_kitti")
    return out


# ---- a3 ----------------------------------------------------------------------------------------------------------
def support_buffer(H, W, device):
    """An empty support plane (see cross_arms): the [H,W] view of a mccnn_support_bytes(H, W) allocation."""
    nbytes = int(hip.load().mccnn_support_bytes(H, W))
    buf = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=device)
    return buf[:H * W].view(H, W)


def cross_arms(image, intensity_threshold, distance_threshold, out=None):
    """image [H,W] -> support plane, int32 [H,W]: one packed word per pixel (mccnn_support_t: bits 0-4 up, 5-9 down,
    10-14 left, 15-19 right, 20-31 region size).  support_arms()/support_count() decode it.  The returned tensor is
    a view of the first plane of a mccnn_support_bytes(H, W) buffer; the derived planes (the words the streaming
    CBCA kernel reads) live behind it in the same storage and travel with the view.  `out`: a support_buffer()."""
    H, W = image.shape
    support = out if out is not None else support_buffer(H, W, image.device)
    hip.check(hip.load().mccnn_cross_arms(hip.ptr(image), H, W, _f32(intensity_threshold), int(distance_threshold),
                                          hip.ptr(support), hip.stream()), "mccnn_cross_arms")
    return support


def cross_arms_pair(image_l, image_r, intensity_threshold, distance_threshold, out_l=None, out_r=None):
    """cross_arms() on both views in one call (half the launches); returns (support_l, support_r)."""
    H, W = image_l.shape
    if tuple(image_r.shape) != (H, W):
        raise ValueError("cross_arms_pair: the two images must have the same shape")
    sl = out_l if out_l is not None else support_buffer(H, W, image_l.device)
    sr = out_r if out_r is not None else support_buffer(H, W, image_l.device)
    hip.check(hip.load().mccnn_cross_arms_pair(hip.ptr(image_l), hip.ptr(image_r), H, W, _f32(intensity_threshold),
                                               int(distance_threshold), hip.ptr(sl), hip.ptr(sr), hip.stream()),
              "mccnn_cross_arms_pair")
    return sl, sr


def support_arms(support):
    """uint8 [H,W,4]: up, down, left, right."""
    s = support.to(torch.int64) & 0xFFFFFFFF
    return torch.stack([(s >> sh) & 31 for sh in (0, 5, 10, 15)], dim=-1).to(torch.uint8)


def support_count(support):
    """int32 [H,W] region sizes (the reference's union_region_num)."""
    return (((support.to(torch.int64) & 0xFFFFFFFF) >> 20) & 0xFFF).to(torch.int32)


def cross_region_list(support, distance_threshold):
    H, W = support.shape
    L = int(distance_threshold)
    region = torch.empty((H, W, (2 * L) ** 2, 2), dtype=torch.int32, device=support.device)
    hip.check(hip.load().mccnn_cross_region_list(hip.ptr(support), H, W, L, hip.ptr(region), hip.stream()),
              "mccnn_cross_region_list")
    return region


# ---- a4 ----------------------------------------------------------------------------------------------------------
def _check_support(support, H, W, who):
    have = support.untyped_storage().nbytes() - support.storage_offset() * support.element_size()
    if tuple(support.shape) != (H, W) or not support.is_contiguous() or have < hip.load().mccnn_support_bytes(H, W):
        raise ValueError("%s: `support` must be the tensor cross_arms() returned (a copy drops its derived planes)" % who)


def cbca(vol, tmp, support, iterations, distance_threshold, order=hip.MCCNN_CBCA_SEPARABLE, timer=None):
    """`iterations` rounds of cross-based averaging.  Ping-pongs between `vol` and `tmp` (same shape);
    returns (result, spare) - the input buffer is clobbered when iterations >= 2, the reference's is not, so
    callers that need the input keep their own copy."""
    D, H, W = vol.shape
    lib = hip.load()
    _check_support(support, H, W, "cbca")
    src, dst = vol, tmp
    timer = timer or _NO_TIMER
    for _ in range(int(iterations)):
        timer.start("cbca_iter")
        hip.check(lib.mccnn_cbca_iter(hip.ptr(src), hip.ptr(dst), hip.ptr(support), D, H, W,
                                      int(distance_threshold), int(order), hip.stream()), "mccnn_cbca_iter")
        timer.stop()
        src, dst = dst, src
    return src, dst


def cbca_pair(vol_l, tmp_l, support_l, vol_r, tmp_r, support_r, iterations, distance_threshold,
              order=hip.MCCNN_CBCA_SEPARABLE, timer=None):
    """cbca() on the left and the right volume together: every iteration is ONE launch that deals the work items of
    both volumes from one pool (mccnn_cbca_iter_pair; same results as two cbca() calls, fewer and fuller rounds of
    workgroups).  Returns ((result_l, spare_l), (result_r, spare_r))."""
    D, H, W = vol_l.shape
    if tuple(vol_r.shape) != (D, H, W):
        raise ValueError("cbca_pair: the two volumes must have the same shape")
    lib = hip.load()
    _check_support(support_l, H, W, "cbca_pair")
    _check_support(support_r, H, W, "cbca_pair")
    (sl, dl), (sr, dr) = (vol_l, tmp_l), (vol_r, tmp_r)
    timer = timer or _NO_TIMER
    for _ in range(int(iterations)):
        timer.start("cbca_iter_pair")
        hip.check(lib.mccnn_cbca_iter_pair(hip.ptr(sl), hip.ptr(dl), hip.ptr(support_l), hip.ptr(sr), hip.ptr(dr),
                                           hip.ptr(support_r), D, H, W, int(distance_threshold), int(order),
                                           hip.stream()), "mccnn_cbca_iter_pair")
        timer.stop()
        sl, dl, sr, dr = dl, sl, dr, sr
    return (sl, dl), (sr, dr)


CBCA_HWD_MAX_DISTANCE = 14     # mccnn_cbca_iter_hwd* and the aggregation programs: arms up to 13
CBCA_MAX_DISTANCE = 32         # the support word's 5-bit arms (mccnn_cross_arms, mccnn_cbca_iter_hwd_long*)


def aggregation_route(distance, W, D, order=hip.MCCNN_CBCA_REFERENCE_ORDER, extras=None, layout="auto",
                      cbca_kernel="auto", H=1):
    """Which aggregation kernel a pair takes - the one decision StereoMatcher, workspace_bytes' callers and
    process_functional share.  Needs no device (only the library's host-side shape rule).  Returns
        "plane_major"  layout="plane_major", the separable order or two-view regions: every stage on [D,H,W]
        "prog"         pixel-major, distance <= 14, and the aggregation programs encode the shape (and cbca_kernel
                       is not "hwd")
        "hwd"          pixel-major, distance <= 14 otherwise (mccnn_cbca_iter_hwd_pair)
        "hwd_long"     pixel-major, 15 <= distance <= 32 (mccnn_cbca_iter_hwd_long_pair; no program buffers)
    and raises ValueError for a distance outside [1, CBCA_MAX_DISTANCE]."""
    distance = int(distance)
    if distance < 1 or distance > CBCA_MAX_DISTANCE:
        raise ValueError("cbca_distance=%d outside [1, %d]: the support word holds 5-bit arms" % (distance, CBCA_MAX_DISTANCE))
    if layout not in ("auto", "plane_major"):
        raise ValueError("layout must be 'auto' or 'plane_major'")
    if layout != "auto" or order != hip.MCCNN_CBCA_REFERENCE_ORDER or (extras or {}).get("both_view_support"):
        return "plane_major"
    if distance > CBCA_HWD_MAX_DISTANCE:
        return "hwd_long"
    if cbca_kernel != "hwd" and int(hip.load().mccnn_cbca_prog_bytes(int(D), int(H), int(W))) != 0:
        return "prog"
    return "hwd"


def route_cbca_kernel(route, cbca_kernel="auto"):
    """The `cbca_kernel` to hand workspace_bytes for a route: "hwd" where no program buffers are allocated."""
    return "hwd" if route in ("hwd", "hwd_long") else cbca_kernel


def cbca_hwd(vol, tmp, support, D, iterations, distance_threshold, timer=None):
    """`iterations` rounds of cross-based averaging in the reference's summation order (bit-exact) on a pixel-major
    volume [H,W,Dp]: mccnn_cbca_iter_hwd for distances up to CBCA_HWD_MAX_DISTANCE, mccnn_cbca_iter_hwd_long for 15 to
    CBCA_MAX_DISTANCE.  Same ping-pong contract as cbca(): returns (result, spare)."""
    H, W, Dp = vol.shape
    assert Dp == hwd_pitch(D) and tuple(tmp.shape) == (H, W, Dp)
    _check_support(support, H, W, "cbca_hwd")
    lib = hip.load()
    src, dst = vol, tmp
    timer = timer or _NO_TIMER
    name = "mccnn_cbca_iter_hwd" if int(distance_threshold) <= CBCA_HWD_MAX_DISTANCE else "mccnn_cbca_iter_hwd_long"
    for _ in range(int(iterations)):
        timer.start("cbca_iter_hwd")
        hip.check(getattr(lib, name)(hip.ptr(src), hip.ptr(dst), hip.ptr(support), int(D), H, W,
                                     int(distance_threshold), hip.stream()), name)
        timer.stop()
        src, dst = dst, src
    return src, dst


def _check_wta_out(wta_out, H, W, who):
    for t in wta_out:
        if tuple(t.shape) != (H, W) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s: wta_out must be two contiguous float32 [H,W] tensors" % who)


def cbca_hwd_wta_max_d():
    """Largest D whose last aggregation iteration can carry the WTA (one chunk of disparities per wave)."""
    return 256


def cbca_hwd_pair(vol_l, tmp_l, support_l, vol_r, tmp_r, support_r, D, iterations, distance_threshold, timer=None,
                  wta_out=None, store_right=True):
    """cbca_hwd() on the left and the right volume, one launch per iteration (mccnn_cbca_iter_hwd_pair, or
    mccnn_cbca_iter_hwd_long_pair for distances above CBCA_HWD_MAX_DISTANCE - which has no fused-WTA form).
    Returns ((result_l, spare_l), (result_r, spare_r)).  wta_out = (disp_l, disp_r) [H,W] float32: the last iteration
    also writes the WTA disparities of both results (mccnn_cbca_iter_hwd_pair_wta; D <= cbca_hwd_wta_max_d());
    store_right=False then leaves the right result volume unwritten (its returned tensor holds stale data)."""
    H, W, Dp = vol_l.shape
    assert Dp == hwd_pitch(D)
    for t in (tmp_l, vol_r, tmp_r):
        if tuple(t.shape) != (H, W, Dp):
            raise ValueError("cbca_hwd_pair: the volumes must have the same shape")
    _check_support(support_l, H, W, "cbca_hwd_pair")
    _check_support(support_r, H, W, "cbca_hwd_pair")
    lib = hip.load()
    (sl, dl), (sr, dr) = (vol_l, tmp_l), (vol_r, tmp_r)
    timer = timer or _NO_TIMER
    n = int(iterations)
    long_arms = int(distance_threshold) > CBCA_HWD_MAX_DISTANCE
    if wta_out is not None:
        if n < 1 or D > cbca_hwd_wta_max_d() or long_arms:
            raise ValueError("cbca_hwd_pair: the fused WTA needs at least one iteration, D <= %d and a distance <= %d"
                             % (cbca_hwd_wta_max_d(), CBCA_HWD_MAX_DISTANCE))
        _check_wta_out(wta_out, H, W, "cbca_hwd_pair")
    pair_name = "mccnn_cbca_iter_hwd_long_pair" if long_arms else "mccnn_cbca_iter_hwd_pair"
    for it in range(n):
        timer.start("cbca_iter_hwd_pair")
        if wta_out is not None and it == n - 1:
            hip.check(lib.mccnn_cbca_iter_hwd_pair_wta(hip.ptr(sl), hip.ptr(dl), hip.ptr(support_l), hip.ptr(sr),
                                                       hip.ptr(dr), hip.ptr(support_r), int(D), H, W,
                                                       int(distance_threshold), hip.ptr(wta_out[0]), hip.ptr(wta_out[1]),
                                                       1 if store_right else 0, hip.stream()),
                      "mccnn_cbca_iter_hwd_pair_wta")
        else:
            hip.check(getattr(lib, pair_name)(hip.ptr(sl), hip.ptr(dl), hip.ptr(support_l), hip.ptr(sr), hip.ptr(dr),
                                              hip.ptr(support_r), int(D), H, W, int(distance_threshold),
                                              hip.stream()), pair_name)
        timer.stop()
        sl, dl, sr, dr = dl, sl, dr, sr
    return (sl, dl), (sr, dr)


def cbca_prog_buffers(D, H, W, device):
    """Two program buffers (left, right image) for cbca_prog_pair, or None when the shape is outside what the
    program-driven kernels encode (mccnn_cbca_prog_bytes == 0): the caller then stays with cbca_hwd_pair."""
    n = int(hip.load().mccnn_cbca_prog_bytes(int(D), int(H), int(W)))
    if n == 0:
        return None
    return (torch.empty((n // 4,), dtype=torch.int32, device=device), torch.empty((n // 4,), dtype=torch.int32, device=device))


def cbca_prog_build_pair(support_l, support_r, D, distance_threshold, progs, which="both"):
    """Compiles both images' support regions into the per-patch programs of the assembly aggregation kernel: once per
    pair, after cross_arms_pair, for all iterations.  which: "full" (mccnn_cbca_prog_build_pair: what every iteration can
    run), "skip" (mccnn_cbca_prog_build_skip_pair: the second set in the same buffers, which second and later iterations
    run, cbca_prog_pair), "both" (mccnn_cbca_prog_build_both_pair: the two sets from one pass over the support words, one
    launch of about the time of either of the others) or "both_two_launches" (the first two one after the other).  The
    buffers remember which sets they hold: cbca_prog_pair / cbca_prog_chain run the full programs in every iteration of
    buffers built with which="full" alone."""
    H, W = support_l.shape
    _check_support(support_l, H, W, "cbca_prog_build_pair")
    _check_support(support_r, H, W, "cbca_prog_build_pair")
    if which not in ("full", "skip", "both", "both_two_launches"):
        raise ValueError("cbca_prog_build_pair: which must be 'full', 'skip', 'both' or 'both_two_launches'")
    lib = hip.load()
    if which == "both":       # one launch, one pass over the support words for the two sets
        hip.check(lib.mccnn_cbca_prog_build_both_pair(hip.ptr(support_l), hip.ptr(support_r), int(D), H, W,
                                                      int(distance_threshold), hip.ptr(progs[0]), hip.ptr(progs[1]),
                                                      hip.stream()), "mccnn_cbca_prog_build_both_pair")
        _record_built(progs, ("full", "skip"))
        return progs
    for name, fn in (("full", lib.mccnn_cbca_prog_build_pair), ("skip", lib.mccnn_cbca_prog_build_skip_pair)):
        if which in (name, "both_two_launches"):
            hip.check(fn(hip.ptr(support_l), hip.ptr(support_r), int(D), H, W, int(distance_threshold), hip.ptr(progs[0]),
                         hip.ptr(progs[1]), hip.stream()), "mccnn_cbca_prog_build_%spair" % ("skip_" if name == "skip" else ""))
    _record_built(progs, ("full", "skip") if which == "both_two_launches" else (which,))
    return progs


def _record_built(progs, sets):
    """Remembers on the program buffers which sets cbca_prog_build_pair has written into them.  A build of the full
    programs forgets the skip set (it may have come from other support arms); a build of the skip set adds to what is
    there."""
    for p in progs:
        p._cbca_prog_sets = (set(getattr(p, "_cbca_prog_sets", ())) | {"skip"}) if sets == ("skip",) else set(sets)


def _skip_set_built(progs):
    """False when cbca_prog_build_pair built these buffers without the skip set (which="full"): the aggregation then
    runs the full programs in every iteration.  Buffers written through the C ABI alone carry no record and are
    assumed complete (the library refuses a set that was never built)."""
    return all("skip" in getattr(p, "_cbca_prog_sets", ("skip",)) for p in progs)


_RIGHT_STREAMS = {}


def right_stream(device):
    """The stream the right volume's chain of aggregation launches runs on (cbca_prog_pair, right_stream=...)."""
    key = (device.type, device.index)
    if key not in _RIGHT_STREAMS:
        _RIGHT_STREAMS[key] = torch.cuda.Stream(device=device)
    return _RIGHT_STREAMS[key]


# (skip_schedule kind, volumes per launch) -> (entry point, StageTimer name): every launch of the program-driven
# aggregation kernel goes through this table (_prog_launch).  bench.py reads the timer names.
_PROG_LAUNCH = {
    ("full", 1): ("mccnn_cbca_iter_prog", "cbca_iter_prog"),
    ("refresh", 1): ("mccnn_cbca_iter_prog_refresh", "cbca_iter_prog"),
    ("skip", 1): ("mccnn_cbca_iter_prog_skip", "cbca_iter_prog_skip"),
    ("full", 2): ("mccnn_cbca_iter_prog_pair", "cbca_iter_prog_pair"),
    ("refresh", 2): ("mccnn_cbca_iter_prog_pair_refresh", "cbca_iter_prog_pair"),
    ("skip", 2): ("mccnn_cbca_iter_prog_pair_skip", "cbca_iter_prog_pair_skip"),
    ("wta", 2): ("mccnn_cbca_iter_prog_pair_wta", "cbca_iter_prog_pair"),
}


def _prog_launch(kind, volumes, D, distance_threshold, timer, tail=()):
    """One launch from _PROG_LAUNCH on the current stream.  volumes: one (src, dst, support, prog) per volume of the
    launch - one, or the left and the right; tail: the arguments an entry point takes behind the distance."""
    name, timed_as = _PROG_LAUNCH[kind, len(volumes)]
    H, W, _ = volumes[0][0].shape
    timer.start(timed_as)
    hip.check(getattr(hip.load(), name)(*[hip.ptr(t) for volume in volumes for t in volume], int(D), H, W,
                                        int(distance_threshold), *tail, hip.stream()), name)
    timer.stop()


def _prog_launch_wta(left, right, D, distance_threshold, wta_out, store_right, timer):
    """The two-volume launch that carries the WTA: an aggregation's last iteration on the full programs, which also
    writes the disparities of both results to wta_out and, with store_right false, leaves the right result volume
    unwritten.  left / right: (src, dst, support, prog)."""
    H, W, _ = left[0].shape
    _check_wta_out(wta_out, H, W, "cbca_prog_pair")
    _prog_launch("wta", (left, right), D, distance_threshold, timer,
                 (hip.ptr(wta_out[0]), hip.ptr(wta_out[1]), 1 if store_right else 0))


def skip_schedule(n, fused_last, skip_unit_regions=True, refresh_first=True):
    """Which kernel every iteration of an n-iteration aggregation runs: a list of "full", "refresh" (the full kernel that
    also writes unit-region pixels back into its input), "skip" and "wta" (the full kernel fused with a7; fused_last) -
    the kinds of _PROG_LAUNCH.  cbca_prog_pair's docstring has the argument."""
    n = int(n)
    kinds = []
    for it in range(n):
        if fused_last and it == n - 1:
            kinds.append("wta")
        elif not skip_unit_regions or it == 0:
            kinds.append("full")
        elif refresh_first or not (n % 2 == 0 and it == n - 1):
            kinds.append("skip")
        else:
            kinds.append("full")
    # The first iteration's input buffer X keeps v0 at unit-region pixels.  As operands v0 and v1 are interchangeable, so
    # X matters only as the FINAL buffer: n even, and then only if the last iteration is a skip launch (a full / WTA
    # launch rewrites every pixel).  Only then does the first iteration have to refresh X.
    if n >= 2 and n % 2 == 0 and kinds[-1] == "skip":
        kinds[0] = "refresh"
    return kinds


def cbca_prog_pair(vol_l, tmp_l, support_l, vol_r, tmp_r, support_r, progs, D, iterations, distance_threshold, timer=None,
                   wta_out=None, store_right=True, skip_unit_regions=True, right_stream=None, refresh_first=True):
    """cbca_hwd_pair's result (bit for bit) through the program-driven assembly kernel (_PROG_LAUNCH); `progs` from
    cbca_prog_build_pair on the same support buffers and D.  Same ping-pong contract; wta_out / store_right as in
    cbca_hwd_pair (_prog_launch_wta for the last iteration).

    skip_unit_regions: from the SECOND iteration on, pixels whose support region is the pixel itself are left alone (the
    "skip" launches).  Such a pixel gets v1 = (0 + v0) / 1 in the first iteration (pf:156-161 with aver_num = 1), which
    is v0 except that -0.0 becomes +0.0 and a signalling NaN is quieted, and (0 + v1) / 1 = v1 bit for bit ever after.
    The first iteration (full programs) puts v1 into the partner buffer; with refresh_first (default, round 6) and an
    even number of iterations that would otherwise have to end with a full launch, it is a "refresh" launch, which also
    writes v1 back into the input buffer, so that BOTH buffers hold the final value of these pixels and every later
    iteration may skip them, whichever buffer it writes: as a NEIGHBOUR in somebody else's region v0 and v1 give the
    same sum bit for bit (a running sum that started as 0 + x is never -0.0, so adding -0.0 or +0.0 cannot differ; a
    NaN operand gives the same quiet NaN either way), and nothing else reads them - except the caller, from the final
    buffer.  refresh_first=False is round 5's rule: the input buffer keeps v0, so with an even number of iterations -
    the result lands in the input buffer - the last iteration runs the full programs and rewrites every pixel.  The
    iteration that carries the WTA runs the full programs either way.  Same bits everywhere, fewer bytes moved.  NOTE:
    a refresh launch modifies the INPUT volume (v0 -> v1 at unit-region pixels); skip_schedule issues one only for an
    even number of iterations without a fused WTA - where the input buffer is also the result buffer, which holds v1
    there in the end either way.

    right_stream: when given, the two volumes run as two independent chains of ONE-volume launches (cbca_prog_chain) -
    the left chain on the current stream, the right chain on `right_stream`, forked from the current stream here and
    joined to it before returning (or before the WTA-carrying last launch, which stays one two-volume launch).  The
    volumes never meet, so nothing orders the chains against each other, and one chain's launch fills the compute
    units the other's leaves idle while its heaviest patches finish: the same bits, 8.7 % less time for 16 iterations
    at 750x500x256 (profiles/r05_cbca_two_streams.txt)."""
    H, W, Dp = vol_l.shape
    assert Dp == hwd_pitch(D)
    for t in (tmp_l, vol_r, tmp_r):
        if tuple(t.shape) != (H, W, Dp):
            raise ValueError("cbca_prog_pair: the volumes must have the same shape")
    _check_support(support_l, H, W, "cbca_prog_pair")
    _check_support(support_r, H, W, "cbca_prog_pair")
    timer = timer or _NO_TIMER
    n = int(iterations)
    fused = wta_out is not None
    if fused and (n < 1 or D > cbca_hwd_wta_max_d()):
        raise ValueError("cbca_prog_pair: the fused WTA needs at least one iteration and D <= %d" % cbca_hwd_wta_max_d())
    skipping = skip_unit_regions and _skip_set_built(progs)
    (sl, dl), (sr, dr) = (vol_l, tmp_l), (vol_r, tmp_r)
    first = 0
    if right_stream is not None:
        # ---- two chains of one-volume launches (every iteration but a WTA-carrying last one) ----
        first = n - 1 if fused else n
        main = torch.cuda.current_stream()
        right_stream.wait_stream(main)
        ends = []
        for st, vol, tmp, sup, prog in ((main, vol_l, tmp_l, support_l, progs[0]),
                                        (right_stream, vol_r, tmp_r, support_r, progs[1])):
            with torch.cuda.stream(st):
                ends.append(cbca_prog_chain(vol, tmp, sup, prog, D, first, distance_threshold, total=n, fused_last=fused,
                                            skip_unit_regions=skipping, timer=timer, refresh_first=refresh_first))
        main.wait_stream(right_stream)
        (sl, dl), (sr, dr) = ends
    kinds = skip_schedule(n, fused, skipping, refresh_first)
    for it in range(first, n):
        left, right = (sl, dl, support_l, progs[0]), (sr, dr, support_r, progs[1])
        if kinds[it] == "wta":
            _prog_launch_wta(left, right, D, distance_threshold, wta_out, store_right, timer)
        else:
            _prog_launch(kinds[it], (left, right), D, distance_threshold, timer)
        sl, dl, sr, dr = dl, sl, dr, sr
    return (sl, dl), (sr, dr)


def cbca_prog_chain(vol, tmp, support, prog, D, iterations, distance_threshold, first=0, total=None, fused_last=False,
                    skip_unit_regions=True, timer=None, refresh_first=True):
    """Iterations first .. iterations-1 of ONE volume's aggregation on the current stream (the one-volume entries of
    _PROG_LAUNCH; cbca_prog_pair's rule for which iterations leave the unit-region pixels alone, with `total` = the
    length of the whole aggregation and fused_last = its last iteration carries the WTA and is not part of the chain).
    The only loop over one-volume launches."""
    n = int(total if total is not None else iterations)
    kinds = skip_schedule(n, fused_last, skip_unit_regions and _skip_set_built((prog,)), refresh_first)
    src, dst = vol, tmp
    timer = timer or _NO_TIMER
    for it in range(int(first), int(iterations)):
        # (a chain asked to run the WTA iteration all the same runs it as what it is without the WTA: a full launch)
        _prog_launch("full" if kinds[it] == "wta" else kinds[it], ((src, dst, support, prog),), D, distance_threshold, timer)
        src, dst = dst, src
    return src, dst


def cbca_both_views(vol, tmp, support_self, support_other, iterations, distance_threshold, side, timer=None):
    """`iterations` rounds of cross-based averaging with the paper's two-view support regions (opt-in extra, see
    mccnn_cbca_iter_both): arms intersected with the other view's at the partner pixel x -/+ d.  Same ping-pong
    contract as cbca()."""
    D, H, W = vol.shape
    lib = hip.load()
    src, dst = vol, tmp
    timer = timer or _NO_TIMER
    for _ in range(int(iterations)):
        timer.start("cbca_iter_both")
        hip.check(lib.mccnn_cbca_iter_both(hip.ptr(src), hip.ptr(dst), hip.ptr(support_self), hip.ptr(support_other), D, H,
                                           W, int(distance_threshold), int(side), hip.stream()), "mccnn_cbca_iter_both")
        timer.stop()
        src, dst = dst, src
    return src, dst


# ---- a5 / a6 -------------------------------------------------------------------------------------------------------
def hwd_pitch(D):
    return hip.load().mccnn_hwd_pitch(int(D))


def dhw_to_hwd(dhw, hwd=None):
    D, H, W = dhw.shape
    if hwd is None:
        hwd = torch.empty((H, W, hwd_pitch(D)), dtype=torch.float32, device=dhw.device)
    hip.check(hip.load().mccnn_dhw_to_hwd(hip.ptr(dhw), hip.ptr(hwd), D, H, W, hip.stream()), "mccnn_dhw_to_hwd")
    return hwd


def hwd_to_dhw(hwd, D, dhw=None):
    H, W, _ = hwd.shape
    if dhw is None:
        dhw = torch.empty((D, H, W), dtype=torch.float32, device=hwd.device)
    hip.check(hip.load().mccnn_hwd_to_dhw(hip.ptr(hwd), hip.ptr(dhw), int(D), H, W, hip.stream()), "mccnn_hwd_to_dhw")
    return dhw


def sgm_scratch(H, W, D, device):
    n = hip.load().mccnn_sgm_scratch_bytes(H, W, int(D))
    return torch.empty((n,), dtype=torch.uint8, device=device)


def _sgm_arrays(sides, *volume_lists):
    """What the SGM entry points take for their 1 or 2 volumes: (n, the c_int[2] of sides, one c_void_p[2] per volume
    list), the unused second slots zero."""
    n = len(volume_lists[0])
    return (n, (ctypes.c_int * 2)(*(list(sides) + [0] * (2 - n)))) + tuple(
        (ctypes.c_void_p * 2)(*([v.data_ptr() for v in vols] + [None] * (2 - n))) for vols in volume_lists)


def _sgm_penalties(sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V):
    """The float32 scalars of the SGM passes: (P1 along a row, P1 along a column = P1 / V in Python double division
    rounded once (pf:204), P2, Q1, Q2, the intensity threshold D)."""
    return _f32(sgm_P1), _f32(sgm_P1 / sgm_V), _f32(sgm_P2), _f32(sgm_Q1), _f32(sgm_Q2), _f32(sgm_D)


def _sgm_p1(r, p1h, p1v):
    return p1h if r[0] == 0 else p1v


def sgm_pass_hwd(image_left, image_right, vols_hwd, sides, D, r, p1, p2, q1, q2, thr, scratch):
    """One direction, in place on 1 or 2 HWD volumes.  p1..thr are already float32-rounded Python floats."""
    H, W = image_left.shape
    n, side_arr, vol_arr = _sgm_arrays(sides, vols_hwd)
    hip.check(hip.load().mccnn_sgm_pass(hip.ptr(image_left), hip.ptr(image_right), vol_arr, side_arr, n, int(D), H, W,
                                        int(r[0]), int(r[1]), p1, p2, q1, q2, thr, hip.ptr(scratch),
                                        scratch.numel(), hip.stream()), "mccnn_sgm_pass")


SGM_DIRECTIONS = ((0, 1), (0, -1), (-1, 0), (1, 0))  # right, left, up, bottom (pf:194-208)


def sgm_flags_hwd(image_left, image_right, D, r, thr, flags):
    """The flag planes of one direction into `flags` (mccnn_sgm_flags); thr is already float32-rounded."""
    H, W = image_left.shape
    hip.check(hip.load().mccnn_sgm_flags(hip.ptr(image_left), hip.ptr(image_right), int(D), H, W, int(r[0]), int(r[1]), thr,
                                         hip.ptr(flags), flags.numel(), hip.stream()), "mccnn_sgm_flags")


def sgm_flag_planes(image_left, image_right, D, sgm_D, out=None):
    """The flag planes of all four directions (mccnn_sgm_flags: which pixels' intensity step along r reaches sgm_D,
    pf:504-533), one buffer per direction: they depend on the images only, so a pair builds them once - off the critical
    path - and every pass of both volumes reads them (sgm_average_hwd(flags=...))."""
    H, W = image_left.shape
    planes = out if out is not None else [sgm_scratch(H, W, D, image_left.device) for _ in SGM_DIRECTIONS]
    for r, buf in zip(SGM_DIRECTIONS, planes):
        sgm_flags_hwd(image_left, image_right, D, r, _f32(sgm_D), buf)
    return planes


def sgm_pass_flagged_hwd(vols_hwd, sides, D, r, p1, p2, q1, q2, flags):
    """One direction, in place on 1 or 2 HWD volumes, with the direction's flag planes already built (sgm_flag_planes)."""
    H, W, _ = vols_hwd[0].shape
    n, side_arr, vol_arr = _sgm_arrays(sides, vols_hwd)
    hip.check(hip.load().mccnn_sgm_pass_flagged(vol_arr, side_arr, n, int(D), H, W, int(r[0]), int(r[1]), p1, p2, q1, q2,
                                                hip.ptr(flags), flags.numel(), hip.stream()), "mccnn_sgm_pass_flagged")


def sgm_average_hwd(image_left, image_right, vols_hwd, sides, D, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V,
                    scratch, timer=_NO_TIMER, flags=None):
    """SGM_average (pf:187-235) on HWD volumes: the four passes compose in place (the reference aliases one array,
    pf:544,568) and its '(a+b+c+d)/4.' of four aliases of that array is the identity in binary floating point
    (the CPU checker used by the tests evaluates it literally; the parity tests pin the equality).
    flags: sgm_flag_planes() of the same images, D and sgm_D - the passes then launch no flag kernels of their own
    (`scratch` is not used)."""
    p1h, p1v, p2, q1, q2, thr = _sgm_penalties(sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V)
    for i, r in enumerate(SGM_DIRECTIONS):
        # (a launch that advances ONE volume - the free-running chains of StereoMatcher - is priced apart from the
        # two-volume launch: half the bytes, and it runs beside whatever the other volume's chain is doing)
        timer.start("sgm_pass" if len(vols_hwd) == 2 else "sgm_pass_one_volume")
        if flags is not None:
            sgm_pass_flagged_hwd(vols_hwd, sides, D, r, _sgm_p1(r, p1h, p1v), p2, q1, q2, flags[i])
        else:
            sgm_pass_hwd(image_left, image_right, vols_hwd, sides, D, r, _sgm_p1(r, p1h, p1v), p2, q1, q2, thr, scratch)
        timer.stop()


def sgm_pass_accumulate_hwd(srcs_hwd, accs_hwd, sides, D, r, p1, p2, q1, q2, mode, flags):
    """One direction out of place on 1 or 2 HWD volumes (mccnn_sgm_pass_accumulate): the costs come from `srcs_hwd`,
    which are not written, and every line of the direction's L is combined with `accs_hwd` as `mode` says
    (hip.MCCNN_SGM_ACC_STORE / _ADD / _ADD_QUARTER).  flags: the direction's planes (sgm_flag_planes)."""
    H, W, _ = srcs_hwd[0].shape
    n, side_arr, src_arr, acc_arr = _sgm_arrays(sides, srcs_hwd, accs_hwd)
    hip.check(hip.load().mccnn_sgm_pass_accumulate(src_arr, acc_arr, side_arr, n, int(D), H, W, int(r[0]), int(r[1]), p1,
                                                   p2, q1, q2, int(mode), hip.ptr(flags), flags.numel(), hip.stream()),
              "mccnn_sgm_pass_accumulate")


SGM_ACC_MODES = (hip.MCCNN_SGM_ACC_STORE, hip.MCCNN_SGM_ACC_ADD, hip.MCCNN_SGM_ACC_ADD, hip.MCCNN_SGM_ACC_ADD_QUARTER)


def sgm_average_independent_hwd(image_left, image_right, vols_hwd, spares_hwd, sides, D, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2,
                                sgm_D, sgm_V, scratch, timer=_NO_TIMER, flags=None):
    """The paper's SGM on HWD volumes: the four directions of SGM_DIRECTIONS each computed from the SAME volume and
    averaged, (((L0 + L1) + L2) + L3) / 4. in float32 - what pf:195-210 spells and, because semi_global_matching
    returns its argument, does not compute (sgm_average_hwd is what it computes).  Four out-of-place passes read
    `vols_hwd` (left unmodified) and accumulate into `spares_hwd`: store, add, add, add-and-quarter.  Returns
    (results, spares) with the roles swapped: the results are the former spares, the former inputs are now spare.
    flags: sgm_flag_planes() of the same images, D and sgm_D; without them every direction's planes are built into
    `scratch` in front of its pass."""
    p1h, p1v, p2, q1, q2, thr = _sgm_penalties(sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V)
    for i, (r, mode) in enumerate(zip(SGM_DIRECTIONS, SGM_ACC_MODES)):
        timer.start("sgm_pass_accumulate" if len(vols_hwd) == 2 else "sgm_pass_accumulate_one_volume")
        planes = flags[i] if flags is not None else scratch
        if flags is None:
            sgm_flags_hwd(image_left, image_right, D, r, thr, scratch)
        sgm_pass_accumulate_hwd(vols_hwd, spares_hwd, sides, D, r, _sgm_p1(r, p1h, p1v), p2, q1, q2, mode, planes)
        timer.stop()
    return list(spares_hwd), list(vols_hwd)


SGM_FIRST_PASS_MAX_D = 256  # mccnn_sgm_first_pass gathers one [256 d][16 w] tile per wave


def sgm_average_from_dhw(image_left, image_right, vols_dhw, vols_hwd, sides, D, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D,
                         sgm_V, scratch, timer=_NO_TIMER):
    """SGM_average starting from plane-major volumes: the first direction (0,1) reads `vols_dhw` and writes the
    pixel-major `vols_hwd` (mccnn_sgm_first_pass: layout change fused into the pass), the other three run in place on
    `vols_hwd`.  For D > 256 the layout change is a separate launch."""
    H, W = image_left.shape
    p1h, p1v, p2, q1, q2, thr = _sgm_penalties(sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V)
    rest = SGM_DIRECTIONS
    if D <= SGM_FIRST_PASS_MAX_D:
        n, side_arr, src, dst = _sgm_arrays(sides, vols_dhw, vols_hwd)
        timer.start("sgm_first_pass")
        hip.check(hip.load().mccnn_sgm_first_pass(hip.ptr(image_left), hip.ptr(image_right), src, dst, side_arr, n,
                                                  int(D), H, W, p1h, p2, q1, q2, thr, hip.ptr(scratch),
                                                  scratch.numel(), hip.stream()), "mccnn_sgm_first_pass")
        timer.stop()
        rest = SGM_DIRECTIONS[1:]
    else:
        timer.start("dhw_to_hwd")
        for a, b in zip(vols_dhw, vols_hwd):
            dhw_to_hwd(a, b)
        timer.stop()
    for r in rest:
        timer.start("sgm_pass")
        sgm_pass_hwd(image_left, image_right, vols_hwd, sides, D, r, _sgm_p1(r, p1h, p1v), p2, q1, q2, thr, scratch)
        timer.stop()


# ---- a7 .. a11 -----------------------------------------------------------------------------------------------------
def wta(vol, out=None):
    D, H, W = vol.shape
    disp = out if out is not None else torch.empty((H, W), dtype=torch.float32, device=vol.device)
    hip.check(hip.load().mccnn_wta(hip.ptr(vol), D, H, W, hip.ptr(disp), hip.stream()), "mccnn_wta")
    return disp


def wta_hwd(vol_hwd, D, out=None):
    """wta() on a pixel-major volume [H,W,Dp]."""
    H, W, Dp = vol_hwd.shape
    assert Dp == hwd_pitch(D)
    disp = out if out is not None else torch.empty((H, W), dtype=torch.float32, device=vol_hwd.device)
    hip.check(hip.load().mccnn_wta_hwd(hip.ptr(vol_hwd), int(D), H, W, hip.ptr(disp), hip.stream()), "mccnn_wta_hwd")
    return disp


def wta_any(vol, D, pixel_major, out=None):
    """wta_hwd() or wta(), as the volume's layout asks."""
    return wta_hwd(vol, D, out=out) if pixel_major else wta(vol, out=out)


def subpixel_hwd(dl, vol_hwd, D, out=None, numpy1_promotion=False):
    """subpixel() on a pixel-major volume [H,W,Dp]."""
    H, W, Dp = vol_hwd.shape
    assert Dp == hwd_pitch(D)
    out = out if out is not None else torch.empty_like(dl)
    hip.check(hip.load().mccnn_subpixel_hwd(hip.ptr(dl), hip.ptr(vol_hwd), int(D), H, W, 1 if numpy1_promotion else 0,
                                            hip.ptr(out), hip.stream()), "mccnn_subpixel_hwd")
    return out


# ---- confidence measures of the left disparity (include/mccnn.h has the definitions) ------------------------------------
CONFIDENCE_MEASURES = ("msm", "mmn", "cur", "lrc")        # in bit order: the order of the planes
_CONFIDENCE_BITS = dict(msm=hip.MCCNN_CONF_MSM, mmn=hip.MCCNN_CONF_MMN, cur=hip.MCCNN_CONF_CUR, lrc=hip.MCCNN_CONF_LRC)


def confidence_mask(names):
    """The MCCNN_CONF_* mask of a sequence of measure names (a single name may be passed as a string).  Unknown and
    repeated names and an empty selection are refused."""
    names = (names,) if isinstance(names, str) else tuple(names)
    mask = 0
    for name in names:
        bit = _CONFIDENCE_BITS.get(name)
        if bit is None:
            raise ValueError("unknown confidence measure %r: choose from %s" % (name, ", ".join(CONFIDENCE_MEASURES)))
        if mask & bit:
            raise ValueError("confidence measure %r named twice" % (name,))
        mask |= bit
    if not mask:
        raise ValueError("no confidence measure named: choose from %s" % ", ".join(CONFIDENCE_MEASURES))
    return mask


def confidence_names(measures):
    """The measures of a selection (names or a mask) in plane order."""
    mask = measures if isinstance(measures, int) else confidence_mask(measures)
    return tuple(n for n in CONFIDENCE_MEASURES if mask & _CONFIDENCE_BITS[n])


VIEW_SUFFIX = {"left": "", "right": "_right"}     # view= of the wrappers below -> what the entry's name carries


def _view_suffix(view):
    if view not in VIEW_SUFFIX:
        raise ValueError("view must be 'left' or 'right'")
    return VIEW_SUFFIX[view]


def _confidence(entry, vol, D, H, W, disp_other, measures, out):
    mask = confidence_mask(measures)
    k = bin(mask).count("1")
    if mask & hip.MCCNN_CONF_LRC and disp_other is None:
        raise ValueError("%s: the lrc measure needs the other view's disparity map" % entry)
    if disp_other is not None and (tuple(disp_other.shape) != (H, W) or disp_other.dtype != torch.float32):
        raise ValueError("%s: the other view's disparity must be a float32 [H,W] map" % entry)
    if vol.dtype != torch.float32:
        raise ValueError("%s: the volume must be float32" % entry)
    if out is None:
        out = torch.empty((k, H, W), dtype=torch.float32, device=vol.device)
    elif tuple(out.shape) != (k, H, W) or out.dtype != torch.float32:
        raise ValueError("%s: `out` must be a float32 [%d,%d,%d] tensor" % (entry, k, H, W))
    hip.check(getattr(hip.load(), entry)(hip.ptr(vol), hip.ptr(disp_other) if disp_other is not None else None, int(D), H,
                                         W, mask, hip.ptr(out), hip.stream()), entry)
    return out


def confidence_hwd(vol_hwd, D, disp_right=None, measures=CONFIDENCE_MEASURES, out=None, view="left"):
    """Confidence planes [K,H,W] of a pixel-major left volume [H,W,Dp], in the order of CONFIDENCE_MEASURES; disp_right:
    the right winner-take-all map (needed by "lrc" only).  view="right": the RIGHT view's planes - of a pixel-major
    right volume and the LEFT winner-take-all map ("lrc" looks it up at column w + d1)."""
    H, W, Dp = vol_hwd.shape
    assert Dp == hwd_pitch(D)
    return _confidence("mccnn_confidence%s_hwd" % _view_suffix(view), vol_hwd, D, H, W, disp_right, measures, out)


def confidence(vol_dhw, disp_right=None, measures=CONFIDENCE_MEASURES, out=None, view="left"):
    """confidence_hwd() on a plane-major volume [D,H,W]: the same bits."""
    D, H, W = vol_dhw.shape
    return _confidence("mccnn_confidence" + _view_suffix(view), vol_dhw, D, H, W, disp_right, measures, out)


def confidence_any(vol, D, pixel_major, disp_other=None, measures=CONFIDENCE_MEASURES, out=None, view="left"):
    """confidence_hwd() or confidence(), as the volume's layout asks."""
    if pixel_major:
        return confidence_hwd(vol, D, disp_other, measures, out=out, view=view)
    return confidence(vol, disp_other, measures, out=out, view=view)


def confidence_right_hwd(vol_right_hwd, D, disp_left=None, measures=CONFIDENCE_MEASURES, out=None):
    """confidence_hwd(view="right")."""
    return confidence_hwd(vol_right_hwd, D, disp_left, measures, out=out, view="right")


def confidence_right(vol_right_dhw, disp_left=None, measures=CONFIDENCE_MEASURES, out=None):
    """confidence(view="right")."""
    return confidence(vol_right_dhw, disp_left, measures, out=out, view="right")


def lr_status(dl, dr, ndisp, out=None, view="left"):
    """The status of the map `dl` against the other view's `dr`; view="right" (mccnn_lr_status_right): `dl` is the right
    map and `dr` the left one."""
    entry = "mccnn_lr_status" + _view_suffix(view)
    H, W = dl.shape
    st = out if out is not None else torch.empty((H, W), dtype=torch.int32, device=dl.device)
    hip.check(getattr(hip.load(), entry)(hip.ptr(dl), hip.ptr(dr), H, W, int(ndisp), hip.ptr(st), hip.stream()), entry)
    return st


def lr_status_right(dr, dl, ndisp, out=None):
    """lr_status(view="right"): the status of the right map `dr` against the left `dl`."""
    return lr_status(dr, dl, ndisp, out=out, view="right")


def interpolate(dl, status, out=None, directions=4, occlusion_from_left=False, view="left"):
    """directions / occlusion_from_left: the paper's rules the reference leaves out (pf:318, pf:361), opt-in.
    view="right" (mccnn_interpolate_right): `dl` is the right map; occlusions are filled from the left, with
    occlusion_from_left - mirrored - from the right; directions = 16 walks the mirrored ray set."""
    H, W = dl.shape
    out = out if out is not None else torch.empty_like(dl)
    rules = (int(directions), 1 if occlusion_from_left else 0)
    if _view_suffix(view):
        entry = "mccnn_interpolate_right"
    elif rules == (4, 0):
        entry, rules = "mccnn_interpolate", ()      # the reference's rule: the entry without the two arguments
    else:
        entry = "mccnn_interpolate_ex"
    hip.check(getattr(hip.load(), entry)(hip.ptr(dl), hip.ptr(status), H, W, *rules, hip.ptr(out), hip.stream()), entry)
    return out


def interpolate_right(dr, status, out=None, directions=4, occlusion_from_right=False):
    """interpolate(view="right"); occlusion_from_right: the mirror of the occlusion_from_left extra."""
    return interpolate(dr, status, out=out, directions=directions, occlusion_from_left=occlusion_from_right, view="right")


def subpixel(dl, vol, out=None, numpy1_promotion=False):
    """numpy1_promotion: evaluate pf:396 as NumPy < 2 promotes it (float64, rounded once) instead of in float32."""
    D, H, W = vol.shape
    out = out if out is not None else torch.empty_like(dl)
    if numpy1_promotion:
        hip.check(hip.load().mccnn_subpixel_ex(hip.ptr(dl), hip.ptr(vol), D, H, W, 1, hip.ptr(out), hip.stream()),
                  "mccnn_subpixel_ex")
    else:
        hip.check(hip.load().mccnn_subpixel(hip.ptr(dl), hip.ptr(vol), D, H, W, hip.ptr(out), hip.stream()),
                  "mccnn_subpixel")
    return out


def subpixel_any(dl, vol, D, pixel_major, out=None, numpy1_promotion=False):
    """subpixel_hwd() or subpixel(), as the volume's layout asks."""
    if pixel_major:
        return subpixel_hwd(dl, vol, D, out=out, numpy1_promotion=numpy1_promotion)
    return subpixel(dl, vol, out=out, numpy1_promotion=numpy1_promotion)


def median(dl, fh, fw, out=None):
    H, W = dl.shape
    out = out if out is not None else torch.empty_like(dl)
    hip.check(hip.load().mccnn_median(hip.ptr(dl), H, W, int(fh), int(fw), hip.ptr(out), hip.stream()),
              "mccnn_median")
    return out


# ---- semi-dense maps: selection and speckle filter (include/mccnn.h has the definitions; csrc/semi_dense.hip) ----------
DROPPED = float("inf")      # what a dropped pixel holds: Middlebury's "unknown"


def _check_map(t, who, name="the map"):
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError("%s: %s must be a float32 [H,W] tensor, got %s %s" % (who, name, t.dtype, tuple(t.shape)))


def semi_dense_select(disp, status=None, planes=None, plane_names=(), thresholds=None, require_match=False, out=None):
    """mccnn_semi_dense_select: `disp` where it is valid, its `status` word (int32 [H,W]) is 0 if require_match, and every
    plane named in `thresholds` ({measure: min}) reaches its value; +inf elsewhere.  planes: [K,H,W] in the order of
    plane_names, as confidence*() wrote them."""
    who = "semi_dense_select"
    _check_map(disp, who)
    H, W = disp.shape
    thresholds = dict((n, _f32(v)) for n, v in dict(thresholds or {}).items())
    if any(math.isnan(v) for v in thresholds.values()):
        raise ValueError("%s: a NaN threshold" % who)
    plane_names = (plane_names,) if isinstance(plane_names, str) else tuple(plane_names)
    have = confidence_mask(plane_names) if plane_names else 0
    use = confidence_mask(tuple(thresholds)) if thresholds else 0
    missing = [n for n in confidence_names(use) if not _CONFIDENCE_BITS[n] & have] if use else []
    if missing:
        raise ValueError("%s: the rule reads %s, which the planes do not hold" % (who, ", ".join(missing)))
    if use:
        k = bin(have).count("1")
        if planes is None or tuple(planes.shape) != (k, H, W) or planes.dtype != torch.float32:
            raise ValueError("%s: `planes` must be a float32 [%d,%d,%d] tensor" % (who, k, H, W))
    if require_match and (status is None or tuple(status.shape) != (H, W) or status.dtype != torch.int32):
        raise ValueError("%s: require_match needs an int32 [%d,%d] status map" % (who, H, W))
    if out is None:
        out = torch.empty_like(disp)
    elif tuple(out.shape) != (H, W) or out.dtype != torch.float32:
        raise ValueError("%s: `out` must be a float32 [%d,%d] tensor" % (who, H, W))
    mc = (ctypes.c_float * 4)(*[thresholds.get(n, 0.0) for n in CONFIDENCE_MEASURES])
    hip.check(hip.load().mccnn_semi_dense_select(
        hip.ptr(disp), hip.ptr(status) if require_match else None, hip.ptr(planes) if use else None, H, W, have, use, mc,
        1 if require_match else 0, hip.ptr(out), hip.stream()), "mccnn_semi_dense_select")
    return out


def speckle_scratch(H, W, device):
    """Scratch of one speckle_filter() in flight (labels and counts): mccnn_speckle_scratch_bytes(H, W) bytes."""
    nbytes = int(hip.load().mccnn_speckle_scratch_bytes(H, W))
    if not nbytes:
        raise ValueError("speckle_scratch: %d x %d is not a size the labelling takes (H*W <= 2^31 - 1)" % (H, W))
    return torch.empty((nbytes // 4,), dtype=torch.int32, device=device)


def speckle_filter(disp, min_size, max_diff=1.0, out=None, sizes=None, want_out=True, want_sizes=False, scratch=None):
    """mccnn_speckle_filter: -> (out, sizes), each None unless wanted or given.  out: `disp` where the pixel's component -
    4-neighbours both valid and no further apart than max_diff, closed transitively - has at least min_size pixels, +inf
    elsewhere; sizes: int32 [H,W] holding the uint32 component sizes (0 for invalid pixels).  `scratch`: a
    speckle_scratch()."""
    who = "speckle_filter"
    _check_map(disp, who)
    H, W = disp.shape
    if out is None and want_out:
        out = torch.empty_like(disp)
    if sizes is None and want_sizes:
        sizes = torch.empty((H, W), dtype=torch.int32, device=disp.device)
    if out is not None and (tuple(out.shape) != (H, W) or out.dtype != torch.float32):
        raise ValueError("%s: `out` must be a float32 [%d,%d] tensor" % (who, H, W))
    if sizes is not None and (tuple(sizes.shape) != (H, W) or sizes.dtype != torch.int32):
        raise ValueError("%s: `sizes` must be an int32 [%d,%d] tensor (the bits are uint32)" % (who, H, W))
    if int(min_size) != min_size or not 0 <= int(min_size) <= 0xFFFFFFFF:
        raise ValueError("%s: min_size=%r is not a uint32" % (who, min_size))
    scratch = scratch if scratch is not None else speckle_scratch(H, W, disp.device)
    hip.check(hip.load().mccnn_speckle_filter(
        hip.ptr(disp), H, W, _f32(max_diff), int(min_size), hip.ptr(out) if out is not None else None,
        hip.ptr(sizes) if sizes is not None else None, hip.ptr(scratch), scratch.numel() * scratch.element_size(),
        hip.stream()), "mccnn_speckle_filter")
    return out, sizes


def semi_dense(disp, rule, status=None, planes=None, plane_names=(), out=None, selected=None, sizes=None, scratch=None):
    """The semi-dense map of `disp` under `rule` (a SemiDenseRule or its text): speckle_filter(semi_dense_select(disp)).
    `selected`: where the selection goes when a speckle part follows (a [H,W] float32 tensor; allocated if None); `sizes`:
    an int32 [H,W] tensor that receives the component sizes of the selection, if given."""
    rule = SemiDenseRule.parse(rule)
    if rule.speckle is None:
        return semi_dense_select(disp, status, planes, plane_names, rule.thresholds, rule.require_match, out=out)
    # (a rule that is a speckle part alone still selects: the one launch that turns invalid pixels into +inf)
    selected = semi_dense_select(disp, status, planes, plane_names, rule.thresholds, rule.require_match, out=selected)
    return speckle_filter(selected, rule.speckle[0], rule.speckle[1], out=out, sizes=sizes, scratch=scratch)[0]


# ---- metric outputs: the depth plane and the ordered point cloud (include/mccnn.h has the definitions; csrc/reproject.hip)
def depth(disp, calib, out=None):
    """mccnn_depth: Z = f32(fx * baseline) / (disp + doffs) where disp is finite and the denominator positive, +inf
    elsewhere.  calib: a calibration.Calibration or its text."""
    who = "depth"
    _check_map(disp, who)
    H, W = disp.shape
    _fx, _fy, _cx, _cy, fb, doffs = Calibration.parse(calib).scalars()
    if out is None:
        out = torch.empty_like(disp)
    elif tuple(out.shape) != (H, W) or out.dtype != torch.float32:
        raise ValueError("%s: `out` must be a float32 [%d,%d] tensor" % (who, H, W))
    hip.check(hip.load().mccnn_depth(hip.ptr(disp), H, W, fb, doffs, hip.ptr(out), hip.stream()), "mccnn_depth")
    return out


def points_scratch(H, W, device):
    """Scratch of one reproject() in flight (block counts and their totals): mccnn_points_scratch_bytes(H, W) bytes."""
    nbytes = int(hip.load().mccnn_points_scratch_bytes(H, W))
    if not nbytes:
        raise ValueError("points_scratch: %d x %d is not a size the compaction takes (H*W <= 2^31 - 1)" % (H, W))
    return torch.empty((nbytes // 4,), dtype=torch.int32, device=device)


def reproject(disp, calib, max_depth=float("inf"), out=None, n_out=None, scratch=None):
    """mccnn_reproject_points: -> (points, n_points).  points: float32 [H*W,4]; its first n_points records are the pixels
    with a finite Z <= max_depth in raster order, (X, Y, Z, the bits of the uint32 h*W + w); the records behind them are
    not written.  n_points: int32 [1] on the device (the bits are uint32): nothing is read back here.  `scratch`: a
    points_scratch()."""
    who = "reproject"
    _check_map(disp, who)
    H, W = disp.shape
    fx, fy, cx, cy, fb, doffs = Calibration.parse(calib).scalars()
    max_depth = _f32(max_depth)
    if math.isnan(max_depth):
        raise ValueError("%s: max_depth is NaN" % who)
    if out is None:
        out = torch.empty((H * W, 4), dtype=torch.float32, device=disp.device)
    elif tuple(out.shape) != (H * W, 4) or out.dtype != torch.float32:
        raise ValueError("%s: `out` must be a float32 [%d,4] tensor" % (who, H * W))
    if n_out is None:
        n_out = torch.empty((1,), dtype=torch.int32, device=disp.device)
    elif tuple(n_out.shape) != (1,) or n_out.dtype != torch.int32:
        raise ValueError("%s: `n_out` must be an int32 [1] tensor (the bits are uint32)" % who)
    scratch = scratch if scratch is not None else points_scratch(H, W, disp.device)
    hip.check(hip.load().mccnn_reproject_points(
        hip.ptr(disp), H, W, fx, fy, cx, cy, fb, doffs, max_depth, hip.ptr(out), hip.ptr(n_out), hip.ptr(scratch),
        scratch.numel() * scratch.element_size(), hip.stream()), "mccnn_reproject_points")
    return out, n_out


GEOMETRY_KEYS = ("calib", "depth", "points", "max_depth")


def parse_geometry(geometry):
    """StereoMatcher(geometry=...) -> dict(calib: Calibration or None, depth, points: bool, max_depth: float) or None.
    Unknown keys, a request for neither output and a NaN max_depth are refused; the calibration may be handed in later
    (set_calibration) but must be there when a pair is matched."""
    if geometry is None:
        return None
    unknown = set(geometry) - set(GEOMETRY_KEYS)
    if unknown:
        raise ValueError("unknown geometry keys: %s" % sorted(unknown))
    g = dict(calib=None, depth=False, points=False, max_depth=float("inf"))
    g.update(geometry)
    g["depth"], g["points"] = bool(g["depth"]), bool(g["points"])
    if not (g["depth"] or g["points"]):
        raise ValueError("geometry= asks for neither depth nor points")
    g["max_depth"] = float(g["max_depth"])
    if math.isnan(g["max_depth"]):
        raise ValueError("geometry: max_depth is NaN")
    if g["calib"] is not None:
        g["calib"] = Calibration.parse(g["calib"])
    return g


def bilateral_table(filter_height, filter_width, mean, std_dev):
    """The reference's spatial kernel (pf:428-436, util.normal util.py:45-48): float64 evaluation, float32 storage."""
    constant1 = 1. / (np.sqrt(2 * np.pi) * std_dev)
    constant2 = -1. / (2 * std_dev * std_dev)
    center_h = (filter_height - 1) // 2
    center_w = (filter_width - 1) // 2
    tab = np.zeros([filter_height, filter_width], dtype=np.float32)
    for h in range(filter_height):
        for w in range(filter_width):
            x = np.sqrt((h - center_h) ** 2 + (w - center_w) ** 2)
            tab[h, w] = constant1 * np.exp(constant2 * ((x - mean) ** 2))
    return tab


_TABLES = {}   # (fh, fw, mean, std_dev, device) -> device table: built once, not per pair


def bilateral_table_device(fh, fw, mean, std_dev, device):
    key = (int(fh), int(fw), float(mean), float(std_dev), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        tab = torch.from_numpy(bilateral_table(int(fh), int(fw), mean, std_dev)).to(device)
        _TABLES[key] = tab
    return tab


def bilateral(image, dl, fh, fw, mean, std_dev, blur_threshold, out=None):
    H, W = dl.shape
    tab = bilateral_table_device(fh, fw, mean, std_dev, dl.device)
    out = out if out is not None else torch.empty_like(dl)
    hip.check(hip.load().mccnn_bilateral(hip.ptr(image), hip.ptr(dl), H, W, int(fh), int(fw), hip.ptr(tab),
                                         _f32(blur_threshold), hip.ptr(out), hip.stream()), "mccnn_bilateral")
    return out


# ---- whole pair ----------------------------------------------------------------------------------------------------
DEFAULT_HP = dict(cbca_intensity=0.02, cbca_distance=14, cbca_num_iterations1=2, cbca_num_iterations2=16,
                  sgm_P1=2.3, sgm_P2=55.9, sgm_Q1=4, sgm_Q2=8, sgm_D=0.08, sgm_V=1.5, blur_sigma=6,
                  blur_threshold=2)  # match.py:32-43


SGM_MAX_D = 1024               # mccnn_sgm_pass: four 256-disparity groups per lane
COST_VOLUME_HWD_MAX_D = 1024   # mccnn_cost_volume_hwd (larger D: the plane-major volume + a layout change)
# What decision="auto" runs where the decision kernel serves the pair (tools/bench_accurate.py, profiles/accurate.json:
# the hand-written kernel is the default only while it is not slower than the library route)
DECISION_AUTO = "kernel"


VIEWS = ("left", "both")       # StereoMatcher(views=...): the left map alone, or [2,H,W] = left, right
# What StereoMatcher._post_view runs on for one view.  name / suffix: the wrappers' view= and what the view's keep= keys and
# timer entries carry (VIEW_SUFFIX); image, own / other (the view's and the other view's WTA map), volume (the view's
# result volume): the inputs; status (None: a fresh tensor), maps (three planes: interp, subpixel, median), dst (the final
# map) and planes (the confidence planes; None without measures): where the results go; stream: where it runs; semi (None
# without a semi-dense rule): the sparse map, the selection, the size plane and the labelling scratch of the view.
PostView = collections.namedtuple("PostView", "name suffix image own other volume status maps dst planes stream semi",
                                  defaults=(None,))


def check_envelope(H, W, D):
    """Raises ValueError for a pair shape the kernels do not serve: 2 <= D <= SGM_MAX_D and D <= W - 2 (the reference's
    border rule).  Volumes of any size within device memory are served (SGM rebases past 4 GiB)."""
    H, W, D = int(H), int(W), int(D)
    if H < 1 or W < 1:
        raise ValueError("%dx%d: empty image" % (W, H))
    if D < 2 or D > SGM_MAX_D:
        raise ValueError("ndisp=%d outside [2, %d]: SGM is built for at most %d disparities" % (D, SGM_MAX_D, SGM_MAX_D))
    if D > W - 2:
        raise ValueError("ndisp=%d needs an image at least ndisp + 2 = %d pixels wide, got W=%d" % (D, D + 2, W))


def workspace_bytes(H, W, D, pixel_major=True, cbca_kernel="auto", pairs_in_flight=1, arch="fast",
                    fc_units=DECISION_UNITS, confidence=0, views="left", semi_dense=False, vertical_offset=0,
                    vertical_offset_max=4, vertical_offset_rows=8, depth=False, points=False, vertical_offset_grid=(3, 4)):
    """Device bytes StereoMatcher.workspace(H, W, D) allocates, times `pairs_in_flight` (match.py --pairs_in_flight:
    one matcher per pair in flight): four volumes of H*W*Dp*4 bytes (Dp = hwd_pitch(D)), the SGM scratch and the flag
    planes of the four directions, both support planes, the status and map planes, and - on pixel-major volumes with
    cbca_kernel != "hwd" - the two aggregation program buffers where their programs encode the shape.  Not included:
    the feature maps (2 x H*W*64*4 bytes while the cost volume is built) and the conv activations.
    arch="accurate": plus the two [H,W,fc_units] float32 halves of the first fully-connected layer.
    confidence: the number K of confidence planes the matcher was asked for (StereoMatcher(confidence=...)): plus one
    [K,H,W] float32 buffer; 0 (default): none.
    views="both" (StereoMatcher(views="both")): plus the right view's status plane, its three intermediate maps, the
    [2,H,W] result and a second set of confidence planes.
    semi_dense (StereoMatcher(semi_dense=...)): plus, per view, two [H,W] float32 maps (the selection and the sparse map),
    the labelling scratch (mccnn_speckle_scratch_bytes) and a [H,W] size plane; False (default): none.
    vertical_offset, vertical_offset_max, vertical_offset_rows (the StereoMatcher extras of these names): with an offset
    other than 0 plus the offset (int32 [1]), the totals (int64 [2 max + 1]) and the votes (int32 [n_rows, ceil(W / 64),
    2 max + 1]); 0 (default): none.  vertical_offset="grid" with vertical_offset_grid=(gh, gw): plus the field (int32) and
    the cells' totals (int64 [2 max + 1] each) of the grid as vertical_field_grid clamps it for this shape.
    depth, points (StereoMatcher(geometry=dict(depth=..., points=...))): plus the [H,W] float32 depth plane; plus the
    [H*W,4] float32 records, the compaction's scratch (mccnn_points_scratch_bytes) and the 4 bytes of their number; False
    (default): none.  Left view only, whatever `views` is."""
    check_envelope(H, W, D)
    if views not in VIEWS:
        raise ValueError("views must be 'left' or 'both'")
    lib = hip.load()
    H, W, D = int(H), int(W), int(D)
    dp = (D + 3) & ~3
    n = 4 * H * W * dp * 4
    n += 5 * int(lib.mccnn_sgm_scratch_bytes(H, W, D))
    n += 2 * int(lib.mccnn_support_bytes(H, W))
    n += H * W * 4 + 6 * H * W * 4
    if pixel_major and cbca_kernel != "hwd":
        n += 2 * int(lib.mccnn_cbca_prog_bytes(D, H, W))
    if arch not in ("fast", "accurate"):
        raise ValueError("arch must be 'fast' or 'accurate'")
    if arch == "accurate":
        n += 2 * H * W * int(fc_units) * 4
    n += int(confidence) * H * W * 4
    if views == "both":
        n += (1 + 3 + 2 + int(confidence)) * H * W * 4
    if semi_dense:
        n += (2 if views == "both" else 1) * (3 * H * W * 4 + int(lib.mccnn_speckle_scratch_bytes(H, W)))
    if vertical_offset != 0:
        rows, blocks, nk = vertical_profile_shape(H, W, vertical_offset_max, vertical_offset_rows)
        n += 4 + 8 * nk + 4 * rows * blocks * nk
        if vertical_offset == "grid":
            gh, gw = vertical_field_grid(H, W, vertical_offset_grid, vertical_offset_rows)
            n += gh * gw * (4 + 8 * nk)
    if depth:
        n += H * W * 4
    if points:
        n += H * W * 16 + int(lib.mccnn_points_scratch_bytes(H, W)) + 4
    return n * max(1, int(pairs_in_flight))


def _require_device_memory(nbytes, what):
    """Raises RuntimeError (before anything is allocated) when `nbytes` exceed the device memory that is free or held
    idle by the caching allocator."""
    free, _total = torch.cuda.mem_get_info()
    avail = free + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if nbytes > avail:
        raise RuntimeError("%s needs %.2f GB of device memory, %.2f GB are available" % (what, nbytes / 1e9, avail / 1e9))


class StereoMatcher(object):
    """The timed region of match.py:129-179 for one stereo pair, resident on one GPU.

    net: model.NET with weights loaded (kept resident; the reference re-restores per pair, pf:43), or a
    model.ACCURATE_NET: its cost volume comes from the decision network (cost_volume_accurate; `decision` selects the
    hand-written kernel or the float32 library route, cv_mode the kernel's precision), every later stage is the same.
    cv_mode / cbca_order select the bit-exact (default, like process_functional and match.py) or the fast,
    tolerance-bounded variant of those two stages.  NOTE (round 3 on): the defaults are the bit-exact variants
    (MCCNN_CV_EXACT, MCCNN_CBCA_REFERENCE_ORDER: 13.7 ms per Middlebury-half pair); callers that relied on the
    earlier default (the fast variants, 9.3 ms) must ask for MCCNN_CV_MFMA / MCCNN_CBCA_SEPARABLE explicitly.
    on_saturation: what match() / match_graph() do when the hand-written feature kernels report that an activation
    left the range of their stored records (|x| >= 255.9: the data was clamped, the features of that pair are not
    float32-accurate).  "fallback" (default): the flag is read after every pair - ONE host synchronisation per pair -
    and such a pair is matched again with the float32 library convolutions; "raise": RuntimeError instead; "ignore":
    nothing is read and nothing blocks - for callers that keep several pairs in flight and poll
    features_saturated() themselves (match.py, bench.py).
    """

    def __init__(self, net, hp=None, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER,
                 feature_tile_rows=None, extras=None, features="auto", layout="auto", cbca_kernel="auto",
                 on_saturation="fallback", skip_unit_regions=True, two_chains=True, free_chains=True, refresh_first=True,
                 sgm_flags_once=True, decision="auto", confidence=(), views="left", semi_dense=None, geometry=None):
        self.device = hip.require_device()
        self.net = net
        self.hp = dict(DEFAULT_HP)
        if hp:
            self.hp.update(hp)
        self.cv_mode = cv_mode
        self.cbca_order = cbca_order
        self.feature_tile_rows = feature_tile_rows   # None: whole image; else NET.features_pair_hwc's band height
        # "split_f16": the split-operand matrix-core kernels (conv_mfma.hip; float32-accurate since round 4: as close to
        # a float64 evaluation as the library); "miopen": float32 library convolutions; "auto" (default): the
        # hand-written kernels where the network has their topology (3x3, 64 maps, >= 2 layers) and no row banding
        # is asked for, the library otherwise
        if features not in ("auto", "miopen", "split_f16"):
            raise ValueError("features must be 'auto', 'miopen' or 'split_f16'")
        if features == "split_f16" and feature_tile_rows is not None:
            raise ValueError("row banding is implemented for the library convolutions only")
        if features == "auto":
            features = "split_f16" if (feature_tile_rows is None and net.supports_split_features()) else "miopen"
        self.features = features
        # An ACCURATE_NET (model.py) produces its cost volume with the decision network instead of the dot product;
        # everything behind the cost volume is the same.  decision: "kernel" = csrc/decision_mfma.hip (cv_mode
        # MCCNN_CV_EXACT: split operands, float32-accurate; MCCNN_CV_MFMA: plain f16), "library" = torch matmuls in
        # float32, "auto" = DECISION_AUTO where the kernel serves the network and the shape, the library otherwise
        # (with a warning that names the limit).  Ignored for the fast network.
        if decision not in ("auto", "kernel", "library"):
            raise ValueError("decision must be 'auto', 'kernel' or 'library'")
        self.accurate = hasattr(net, "fc_weights")
        self.decision = decision
        if self.accurate and features == "split_f16":
            raise ValueError("the split-operand feature kernels are built for the fast network")
        # "auto": the bit-exact variant runs on pixel-major volumes (pixel_major()); "plane_major" keeps every stage
        # on the reference's [D,H,W] layout (the round-2 kernels: cross-checks, and what the fast variant always uses)
        if layout not in ("auto", "plane_major"):
            raise ValueError("layout must be 'auto' or 'plane_major'")
        self.layout = layout
        # reference-order aggregation on pixel-major volumes: "prog" = the program-driven assembly kernel
        # (cbca_prog_pair), "hwd" = cbca_hwd_kernel; "auto": the first wherever its programs encode the shape
        if cbca_kernel not in ("auto", "prog", "hwd"):
            raise ValueError("cbca_kernel must be 'auto', 'prog' or 'hwd'")
        self.cbca_kernel = cbca_kernel
        if on_saturation not in ("fallback", "raise", "ignore"):
            raise ValueError("on_saturation must be 'fallback', 'raise' or 'ignore'")
        self.on_saturation = on_saturation
        self._library_twin = None
        self._decision_ran = None          # route of the last accurate cost volume: "kernel" raises the saturation flag
        # cbca_prog_pair's rule (iterations that leave unit-region pixels alone: same bits, fewer bytes); False runs the
        # full programs in every iteration - the content-independent cost of the aggregation (bench.py reports both)
        self.skip_unit_regions = bool(skip_unit_regions)
        # the program-driven aggregation as two chains of one-volume launches on two streams (cbca_prog_pair,
        # right_stream): same bits; False = one two-volume launch per iteration
        self.two_chains = bool(two_chains)
        # free_chains (default since round 6; measured with tools/dev_ab_matchers.py, profiles/r05_ab_matcher_options.txt):
        # each volume's aggregation -> SGM -> aggregation as ONE free-running chain of one-volume launches on its own
        # stream, no join between the stages (-0.10 .. -0.16 ms per cfg2 pair, same bits); False = round 5's schedule: the
        # chains join after every stage and the SGM passes are two-volume launches
        self.free_chains = bool(free_chains)
        # skip_schedule's rule (round 6): an aggregation with an even number of iterations whose last launch carries no WTA
        # (match.py's first: 2 iterations) starts with a refresh launch and then skips to the end; False = round 5's rule
        # (its last launch is a full one)
        self.refresh_first = bool(refresh_first)
        # the SGM flag planes of the four directions built once per pair on the side stream (mccnn_sgm_flags) and read by
        # the passes of both chains; False = every one-volume pass launches its own flag kernel (8 per pair, on the chains)
        self.sgm_flags_once = bool(sgm_flags_once)
        # opt-in departures from the reference (they change the output): the paper's rules it leaves out, and the
        # scalar promotion of the NumPy it was written for
        # sgm_independent_directions: the paper's SGM - the four directions each from the same volume, averaged
        # (sgm_average_independent_hwd) - instead of the reference's four passes composed on one array
        self.extras = dict(both_view_support=False, interpolation_directions=4, occlusion_from_left=False,
                           numpy1_promotion=False, sgm_independent_directions=False, vertical_range=0,
                           vertical_offset=0, vertical_offset_max=4, vertical_offset_rows=8,
                           vertical_offset_grid=(3, 4))
        if extras:
            unknown = set(extras) - set(self.extras)
            if unknown:
                raise ValueError("unknown extras: %s" % sorted(unknown))
            self.extras.update(extras)
        # vertical_range: the cost volume's vertical search for imperfectly rectified pairs (cost_volume_vertical_hwd)
        # in the place of cost_volume_hwd; every later stage is the same.  0 (default): nothing changes - the same
        # launches, workspace and graphs.  Only where the bit-exact dot-product volume is written pixel-major.
        self._check_vertical_range()
        # vertical_offset: the cost volume taken along a row offset of the pair (cost_volume_offset_hwd), vertical_range
        # searched around it.  An integer in [-8, 8] is placed in the workspace once; "auto" measures it per pair on the
        # pair's stream (vertical_profile of +-vertical_offset_max rows on every vertical_offset_rows-th row ->
        # vertical_offset_select -> the volume; no host round trip, capturable); vertical_report() reads the measurement
        # back.  0 (default): nothing changes - no launch, no buffer.  Refused where vertical_range > 0 is.
        # "grid": one offset per cell of vertical_offset_grid = (gh, gw) cells, clamped per shape (vertical_field_grid),
        # for a rolled rig or unequal focal lengths, whose residual averages to nothing: vertical_profile ->
        # vertical_field_select -> cost_volume_field_hwd, on the pair's stream like "auto".
        self._check_vertical_offset()
        # confidence measures of the returned map (CONFIDENCE_MEASURES; names in any order, planes in that order): one
        # more launch per pair behind the post-processing, and every match entry returns (map, planes [K,H,W]).
        # Empty (default): nothing changes - no launch, no buffer, the map alone is returned.
        self.confidence = confidence_names(confidence) if confidence else ()
        # "both": every match entry returns [2,H,W] = the left map (the same bits) and the post-processed RIGHT map
        # (include/mccnn.h: the left rules on the flipped pair, flipped back); confidence planes become [2,K,H,W].  The
        # WTA-carrying launch then stores the right result volume and the right view's a8 .. a11 run beside the left's.
        # "left" (default): nothing changes - the same launches, workspace and graphs.
        if views not in VIEWS:
            raise ValueError("views must be 'left' or 'both'")
        self.views = views
        self.both = views == "both"
        # a SemiDenseRule or its text: every match entry returns the sparse map ([H,W], or [2,H,W] with both views) as
        # the last element of its result, behind the map and the planes: per view one more launch behind the confidence
        # launch (the selection; a rule without a speckle part) or five (the selection and the labelling's four).  The measures the rule reads must be among `confidence`: none is added silently (that would
        # change K).  None (default): nothing changes - no launch, no buffer, the results as they were.
        self.semi_dense = SemiDenseRule.parse(semi_dense) if semi_dense is not None else None
        if self.semi_dense is not None:
            missing = [n for n in self.semi_dense.measures if n not in self.confidence]
            if missing:
                raise ValueError("semi_dense=%r reads the confidence measure %s, which confidence=%r does not produce"
                                 % (self.semi_dense.describe(), ", ".join(missing), self.confidence))
        # dict(calib=a Calibration or its text, depth=bool, points=bool, max_depth=float): the metric outputs of the LEFT
        # view behind everything else on the pair's stream - the depth plane of the dense map (one launch) and / or the
        # ordered point cloud (four launches) of the sparse map where the matcher has a semi-dense rule, of the dense one
        # otherwise; every match entry returns them behind what it returns today: [, depth][, points, n_points].  The
        # calibration is a launch argument: set_calibration() replaces it, and a captured graph is good for the
        # calibration it was captured with (its key carries the scalars).  None (default): nothing changes - no launch,
        # no buffer, the results as they were.
        self.geometry = parse_geometry(geometry)
        self._ws = {}
        self._graphs = {}
        self._side = None
        self._right = None
        self._ingest = None

    def set_calibration(self, calib):
        """The calibration of the pairs that follow (a Calibration or its text): a launch argument of the metric outputs.
        Graphs captured under another calibration stay resident for as long as the shape does and are replayed when that
        calibration comes back; a new one is captured on its first match_graph*()."""
        if self.geometry is None:
            raise ValueError("set_calibration: this matcher has no geometry=")
        self.geometry["calib"] = Calibration.parse(calib)

    def _geometry_kw(self):
        """The workspace_bytes keywords of this matcher's geometry=; empty without it."""
        g = self.geometry
        return dict(depth=g["depth"], points=g["points"]) if g is not None else {}

    def _check_vertical_range(self):
        r = self.extras["vertical_range"]
        if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r <= VERTICAL_RANGE_MAX:
            raise ValueError("vertical_range must be an integer in [0, %d], not %r" % (VERTICAL_RANGE_MAX, r))
        if r == 0:
            return
        if self.accurate:
            raise ValueError("vertical_range=%d: the accurate network's decision stage has no vertical search" % r)
        if self.cv_mode != hip.MCCNN_CV_EXACT:
            raise ValueError("vertical_range=%d: the matrix-core cost volume (MCCNN_CV_MFMA) has no vertical search" % r)
        if not self.pixel_major():
            raise ValueError("vertical_range=%d: the vertical search writes pixel-major volumes, and this configuration's "
                             "cost volume starts plane-major (layout='plane_major', the separable aggregation order or "
                             "both_view_support)" % r)

    def _check_vertical_offset(self):
        v, R, step = (self.extras[k] for k in ("vertical_offset", "vertical_offset_max", "vertical_offset_rows"))
        if v not in ("auto", "grid") and (isinstance(v, bool) or not isinstance(v, int) or abs(v) > VERTICAL_OFFSET_MAX):
            raise ValueError("vertical_offset must be 'auto' or an integer in [-%d, %d] (or 'grid'), not %r"
                             % (VERTICAL_OFFSET_MAX, VERTICAL_OFFSET_MAX, v))
        grid = self.extras["vertical_offset_grid"]
        if not isinstance(grid, (tuple, list)) or len(grid) != 2 or any(
                isinstance(g, bool) or not isinstance(g, int) or not 1 <= g <= VERTICAL_FIELD_MAX for g in grid):
            raise ValueError("vertical_offset_grid must be two integers (gh, gw) in [1, %d], not %r"
                             % (VERTICAL_FIELD_MAX, grid))
        if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= VERTICAL_OFFSET_MAX:
            raise ValueError("vertical_offset_max must be an integer in [1, %d], not %r" % (VERTICAL_OFFSET_MAX, R))
        if isinstance(step, bool) or not isinstance(step, int) or step < 1:
            raise ValueError("vertical_offset_rows must be an integer >= 1, not %r" % (step,))
        if v == 0:
            return
        if self.accurate:
            raise ValueError("vertical_offset=%r: the accurate network's decision stage has no row offset" % (v,))
        if self.cv_mode != hip.MCCNN_CV_EXACT:
            raise ValueError("vertical_offset=%r: the matrix-core cost volume (MCCNN_CV_MFMA) has no row offset" % (v,))
        if not self.pixel_major():
            raise ValueError("vertical_offset=%r: the offset cost volume writes pixel-major volumes, and this "
                             "configuration's cost volume starts plane-major (layout='plane_major', the separable "
                             "aggregation order or both_view_support)" % (v,))

    def _vertical_offset_on(self):
        return self.extras["vertical_offset"] != 0

    def _vertical_field_on(self):
        return self.extras["vertical_offset"] == "grid"

    def vertical_grid(self, H, W):
        """The (gh, gw) cells vertical_offset="grid" uses for an H x W pair: vertical_offset_grid as vertical_field_grid
        clamps it for the shape."""
        return vertical_field_grid(H, W, self.extras["vertical_offset_grid"], self.extras["vertical_offset_rows"])

    def vertical_report(self, H, W, D):
        """The row offset the last pair on the workspace of this shape was matched along: {offset, totals, share} -
        the offset, the votes per candidate -max .. +max and the winner's share of them (an integer vertical_offset has
        no votes: zeros and 0.0).  vertical_offset="grid": plus grid [gh, gw] (as clamped for the shape), offsets
        [gh][gw], cell_totals and cell_shares (vertical_field_record).  Synchronises the device; never call it inside a
        capture."""
        buffers = self.vertical_buffers(H, W, D)
        if buffers is None:
            raise ValueError("vertical_report: no pair of %dx%d, ndisp=%d has been matched with vertical_offset on"
                             % (W, H, D))
        torch.cuda.synchronize()
        if len(buffers) == 4:
            return vertical_field_record(*(b.cpu().numpy() for b in buffers))
        return vertical_record(buffers[0].cpu().numpy(), buffers[1].cpu().numpy())

    def vertical_buffers(self, H, W, D):
        """(offset int32 [1], totals int64 [2 max + 1]) of the resident workspace of this shape - what vertical_report()
        reads, for a caller that copies them out in stream order itself (the list loops) - or None.
        vertical_offset="grid": (offset, totals, field int32 [gh, gw], cell totals int64 [gh, gw, 2 max + 1])."""
        ws = self._ws.get((int(H), int(W), int(D)))
        if ws is None or "v_offset" not in ws:
            return None
        if "v_field" in ws:
            return (ws["v_offset"], ws["v_totals"], ws["v_field"], ws["v_cells"])
        return (ws["v_offset"], ws["v_totals"])

    def _right_stream(self):
        """The stream of the right volume's chain of aggregation launches: this matcher's own (like its side stream), so
        that a stream never meets the captures of two different graphs - a module-wide stream that had been part of
        the capture of a graph destroyed since crashed the runtime in a later capture once in three test runs."""
        if self._right is None:
            self._right = torch.cuda.Stream()
        return self._right

    def features_saturated(self, reset=True):
        """True when the split-operand feature kernels clamped an activation since the last reset (blocks the host)."""
        return self.net.split_saturated(reset)

    def saturation_checked(self):
        """True when the last pair ran a hand-written kernel that raises the saturation flag (the split-operand feature
        kernels of the fast network, the decision kernel of the accurate one): features_saturated() then has news."""
        return self.features == "split_f16" or (self.accurate and self._decision_ran == "kernel")

    def saturation_notice(self):
        """The sentence match.py prints when it repeats a pair whose saturation flag was raised: which kernel's range
        was left and which library route takes the pair."""
        if self.accurate:
            return "activations left the matrix-core decision kernel's range: {} repeated on the float32 library decision route"
        return ("activations left the matrix-core feature kernels' range: {} repeated with the float32 library "
                "convolutions")

    def workspace(self, H, W, D):
        key = (H, W, D)
        ws = self._ws.get(key)
        if ws is None:
            need = workspace_bytes(H, W, D, self.pixel_major(), self.workspace_cbca_kernel(H, W, D),
                                   arch="accurate" if self.accurate else "fast",
                                   fc_units=self.net.num_fc_units if self.accurate else DECISION_UNITS,
                                   confidence=len(self.confidence), views=self.views,
                                   semi_dense=self.semi_dense is not None, **self._geometry_kw(),
                                   **{k: self.extras[k] for k in ("vertical_offset", "vertical_offset_max",
                                                                  "vertical_offset_rows") if self._vertical_offset_on()},
                                   **(dict(vertical_offset_grid=tuple(self.extras["vertical_offset_grid"]))
                                      if self._vertical_field_on() else {}))
            self._ws, self._graphs = {}, {}          # one shape resident at a time: the previous one goes first
            _require_device_memory(need, "StereoMatcher: the workspace of a %dx%d pair with ndisp=%d" % (W, H, D))
            dp = hwd_pitch(D)
            n = H * W * dp                        # >= D*H*W: every volume buffer can hold either layout
            dev = self.device
            ws = dict(
                vol=[torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(4)],
                scratch=sgm_scratch(H, W, D, dev),
                sgm_flags=[sgm_scratch(H, W, D, dev) for _ in SGM_DIRECTIONS],     # flag planes of the four directions
                sup_l=support_buffer(H, W, dev), sup_r=support_buffer(H, W, dev),
                status=torch.empty((H, W), dtype=torch.int32, device=dev),
                maps=torch.empty((6, H, W), dtype=torch.float32, device=dev),   # dl, dr, interp, subpixel, median, out
            )
            if self.accurate:
                ws["halves"] = tuple(torch.empty((H, W, self.net.num_fc_units), dtype=torch.float32, device=dev)
                                     for _ in range(2))
            if self.confidence:
                ws["confidence"] = torch.empty(((2,) if self.both else ()) + (len(self.confidence), H, W),
                                               dtype=torch.float32, device=dev)
            if self.both:
                ws["status_right"] = torch.empty((H, W), dtype=torch.int32, device=dev)
                ws["maps_right"] = torch.empty((3, H, W), dtype=torch.float32, device=dev)   # interp, subpixel, median
                ws["both"] = torch.empty((2, H, W), dtype=torch.float32, device=dev)         # the result: left, right
            if self.semi_dense is not None:
                lead = (2,) if self.both else ()
                ws["sparse"] = torch.empty(lead + (H, W), dtype=torch.float32, device=dev)      # the result
                ws["semi_selected"] = torch.empty(lead + (H, W), dtype=torch.float32, device=dev)
                ws["semi_sizes"] = torch.empty(lead + (H, W), dtype=torch.int32, device=dev)
                ws["semi_scratch"] = [speckle_scratch(H, W, dev) for _ in range(2 if self.both else 1)]
            if self.geometry is not None and self.geometry["depth"]:
                ws["depth"] = torch.empty((H, W), dtype=torch.float32, device=dev)
            if self.geometry is not None and self.geometry["points"]:
                ws["points"] = torch.empty((H * W, 4), dtype=torch.float32, device=dev)
                ws["n_points"] = torch.empty((1,), dtype=torch.int32, device=dev)
                ws["points_scratch"] = points_scratch(H, W, dev)
            if self._vertical_offset_on():
                v, R = self.extras["vertical_offset"], self.extras["vertical_offset_max"]
                ws["v_offset"] = torch.full((1,), 0 if v in ("auto", "grid") else v, dtype=torch.int32, device=dev)
                ws["v_totals"] = torch.zeros((2 * R + 1,), dtype=torch.int64, device=dev)
                ws["v_votes"] = torch.zeros(vertical_profile_shape(H, W, R, self.extras["vertical_offset_rows"]),
                                            dtype=torch.int32, device=dev)
                if self._vertical_field_on():
                    grid = self.vertical_grid(H, W)
                    ws["v_field"] = torch.zeros(grid, dtype=torch.int32, device=dev)
                    ws["v_cells"] = torch.zeros(grid + (2 * R + 1,), dtype=torch.int64, device=dev)
            ws["progs"] = None
            # (distances above CBCA_HWD_MAX_DISTANCE: the aggregation programs do not encode such arms - the joined
            # two-volume path of mccnn_cbca_iter_hwd_long_pair runs, as for shapes the programs do not encode)
            if self.route(H, W, D) == "prog":
                ws["progs"] = cbca_prog_buffers(D, H, W, dev)
            elif self.pixel_major() and self.cbca_kernel == "prog":
                raise ValueError("cbca_kernel='prog': %dx%dx%d (cbca_distance %d) is outside what the aggregation "
                                 "programs encode" % (W, H, D, int(self.hp["cbca_distance"])))
            bilateral_table_device(5, 5, 0, self.hp["blur_sigma"], dev)
            self._ws = {key: ws}  # one shape resident at a time
            self._graphs = {}
        return ws

    def route(self, H, W, D):
        """aggregation_route() of this matcher for a pair shape."""
        return aggregation_route(self.hp["cbca_distance"], W, D, self.cbca_order, self.extras, self.layout,
                                 self.cbca_kernel, H)

    def workspace_cbca_kernel(self, H, W, D):
        """The `cbca_kernel` argument under which workspace_bytes states what workspace() allocates."""
        return route_cbca_kernel(self.route(H, W, D), self.cbca_kernel)

    def pixel_major(self):
        """True when the pair runs on pixel-major volumes from the first aggregation on: the bit-exact variant
        (reference-order CBCA, any distance the support word holds, no two-view regions).  CBCA, SGM, WTA and
        sub-pixel then all work on [H,W,Dp] and no layout change surrounds the SGM stage."""
        return aggregation_route(self.hp["cbca_distance"], 1, 1, self.cbca_order, self.extras, self.layout,
                                 "hwd") != "plane_major"

    def result_of(self, value):
        """What a match entry of this matcher returned, as a PairResult: decoded by the matcher's own configuration."""
        g = self.geometry or dict(depth=False, points=False)
        return PairResult.decode(value, bool(self.confidence), self.semi_dense is not None, g["depth"], g["points"])

    def _saturated_pair(self, left_image, right_image, ndisp, given, keep=None):
        """on_saturation for the pair that has just been launched: None when its features were fine (or nobody is to
        look), else the PairResult of the same pair behind the float32 library convolutions, every field written to
        the tensor `given` (a PairResult of the caller's tensors or None) holds for it.
        keep: the dict the pair's stages were handed out in; the repeated pair's stages replace them."""
        if not self.saturation_checked() or self.on_saturation == "ignore" or torch.cuda.is_current_stream_capturing():
            return None
        if not self.features_saturated():
            return None
        if self.on_saturation == "raise":
            raise RuntimeError("StereoMatcher: an activation left the range of the split-operand %s "
                               "(|x| >= 255.9); match this pair with %s" % (
                                   ("decision kernel", "decision='library'") if self.accurate else
                                   ("feature kernels", "features='miopen'")))
        if self._library_twin is None:
            self._library_twin = StereoMatcher(self.net, hp=self.hp, cv_mode=self.cv_mode, cbca_order=self.cbca_order,
                                               extras=self.extras, features="miopen", layout=self.layout,
                                               cbca_kernel=self.cbca_kernel, on_saturation="ignore", decision="library",
                                               confidence=self.confidence, views=self.views,
                                               semi_dense=self.semi_dense, geometry=self.geometry)
        if self.geometry is not None:
            self._library_twin.geometry["calib"] = self.geometry["calib"]
        if keep is not None:
            keep.clear()
        return self._library_twin._match(left_image, right_image, ndisp, given, keep=keep)   # (it never repeats a pair)

    def match(self, left_image, right_image, ndisp, timer=_NO_TIMER, keep=None, _static_out=False, out=None,
              confidence_out=None, semi_out=None, depth_out=None, points_out=None):
        """_match() + the on_saturation policy (class docstring): a pair whose hand-written features were clamped is
        matched again with the library convolutions unless the caller asked to be left alone.  With `keep` the stages
        handed out are those of the map that is returned: the repeated pair's where the pair was repeated.
        A matcher with confidence measures returns (map, planes [K,H,W]); the planes follow the map's rules - a copy,
        or `confidence_out` (a contiguous float32 [K,H,W] device tensor) where one is given, next to `out`.
        A matcher with a semi-dense rule returns the sparse map as the last element - (map, sparse) or (map, planes,
        sparse) - by the same rules, with `semi_out` (shaped like `out`) in the place of `confidence_out`.
        A matcher with geometry= returns behind those the depth plane ([H,W]; `depth_out`) and / or the cloud's records and
        their number ([H*W,4] float32 and int32 [1] on the device; `points_out` takes the records) - the left view's.
        (PairResult.public() is that shape; result_of() reads it back.)"""
        given = PairResult(out, confidence_out, semi_out, depth_out, points_out)
        res = self._match(left_image, right_image, ndisp, given, timer=timer, keep=keep, _static_out=_static_out)
        redo = None if _static_out else self._saturated_pair(left_image, right_image, ndisp, given, keep)
        return (res if redo is None else redo).public()

    # ---- one pair, stage by stage (_match below is the schedule; INTEGRATION.md has the map) ----
    def _side_work(self, ws, L, R, D, want_flags):
        """What depends on the images only, on the matcher's side stream (forked from the current one): the support arms,
        the aggregation programs where the workspace has buffers for them - both sets from one pass over the support
        words - and, when wanted, the SGM flag planes.  Returns (sup_l, sup_r, flag_planes or None, the event after which
        all of it is complete)."""
        hp = self.hp
        if self._side is None:
            self._side = torch.cuda.Stream()
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            sup_l, sup_r = cross_arms_pair(L, R, hp["cbca_intensity"], hp["cbca_distance"], ws["sup_l"], ws["sup_r"])
            if ws["progs"] is not None:
                cbca_prog_build_pair(sup_l, sup_r, D, hp["cbca_distance"], ws["progs"],
                                     "both" if self.skip_unit_regions else "full")
            flag_planes = sgm_flag_planes(L, R, D, hp["sgm_D"], out=ws["sgm_flags"]) if want_flags else None
            ready = torch.cuda.Event()
            ready.record(self._side)
        return sup_l, sup_r, flag_planes, ready

    def _side_work_timed(self, ws, L, R, D, timer):
        """The arms and the programs of _side_work on the current stream, each under its own timer entry (per-stage
        timing: nothing runs beside anything).  Returns (sup_l, sup_r)."""
        hp = self.hp
        timer.start("cross_arms")
        sup_l, sup_r = cross_arms_pair(L, R, hp["cbca_intensity"], hp["cbca_distance"], ws["sup_l"], ws["sup_r"])
        timer.stop()
        if ws["progs"] is not None:
            timer.start("cbca_prog_build")
            cbca_prog_build_pair(sup_l, sup_r, D, hp["cbca_distance"], ws["progs"])
            timer.stop()
        return sup_l, sup_r

    def decision_route(self, W, D):
        """"kernel" or "library" for an accurate network's pair of this width and disparity range (class docstring of
        __init__: decision).  "auto" falls back to the library, with a warning, where the kernel refuses."""
        if self.decision == "library":
            return "library"
        why = decision_kernel_refusal(self.net, W, D)
        if why is None:
            return DECISION_AUTO if self.decision == "auto" else "kernel"
        if self.decision == "kernel":
            raise ValueError("decision='kernel': %s" % why)
        import warnings
        warnings.warn("accurate network: %s; the decision stage runs on the float32 library route" % why)
        return "library"

    def _cost_volumes_accurate(self, ws, fl, fr, D, dhw, hwd, timer):
        """_cost_volumes for an ACCURATE_NET: the decision network on every (pixel, disparity) pair."""
        direct = self.pixel_major() and D <= COST_VOLUME_HWD_MAX_D
        route = self.decision_route(fl.shape[1], D)
        self._decision_ran = route
        timer.start("cost_volume")
        left, right = cost_volume_accurate(self.net, fl, fr, D, mode=self.cv_mode, decision=route, pixel_major=direct,
                                           out=(hwd[2], hwd[3]) if direct else (dhw[0], dhw[1]), halves=ws["halves"],
                                           sat_flag=self.net._split_flag() if route == "kernel" else None)
        timer.stop()
        return left, right, direct

    def _cost_volumes(self, fl, fr, D, dhw, hwd, timer, ws=None):
        """Returns (left, right, pixel_major): the bit-exact variant writes its cost volume pixel-major right away
        (nothing converts layouts after that) where the kernel serves D; everything else starts plane-major."""
        if self.accurate:
            return self._cost_volumes_accurate(ws, fl, fr, D, dhw, hwd, timer)
        direct = self.pixel_major() and D <= COST_VOLUME_HWD_MAX_D
        vertical = self.extras["vertical_range"]
        if vertical and not direct:
            raise ValueError("vertical_range=%d: the vertical search writes pixel-major volumes of at most %d disparities, "
                             "not %d" % (vertical, COST_VOLUME_HWD_MAX_D, D))
        offset = self.extras["vertical_offset"]
        if offset != 0 and not direct:
            raise ValueError("vertical_offset=%r: the offset cost volume writes pixel-major volumes of at most %d "
                             "disparities, not %d" % (offset, COST_VOLUME_HWD_MAX_D, D))
        timer.start("cost_volume")
        if offset != 0:
            R, step = self.extras["vertical_offset_max"], self.extras["vertical_offset_rows"]
            if offset in ("auto", "grid"):   # measured from this pair's features, on this stream; the kernel reads the result
                votes = vertical_profile(fl, fr, D, R, step, out=ws["v_votes"])
            if offset == "grid":             # ... per cell of the grid the workspace was sized for
                vertical_field_select(votes, fl.shape[0], step, R, tuple(ws["v_field"].shape),
                                      out=(ws["v_field"], ws["v_cells"], ws["v_offset"], ws["v_totals"]))
                left, right = cost_volume_field_hwd(fl, fr, D, ws["v_field"], vertical, out=(hwd[2], hwd[3]))
            else:
                if offset == "auto":
                    vertical_offset_select(votes, R, out=(ws["v_offset"], ws["v_totals"]))
                left, right = cost_volume_offset_hwd(fl, fr, D, ws["v_offset"], vertical, out=(hwd[2], hwd[3]))
        elif vertical:
            left, right = cost_volume_vertical_hwd(fl, fr, D, vertical, out=(hwd[2], hwd[3]))
        elif direct:
            left, right = cost_volume_hwd(fl, fr, D, out=(hwd[2], hwd[3]), mode=self.cv_mode)
        else:
            left, right = cost_volume(fl, fr, D, self.cv_mode, out=(dhw[0], dhw[1]))
        timer.stop()
        return left, right, direct

    def _sgm_hp(self):
        return [self.hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]

    def _wta(self, lv, rv, D, pixel_major, m, timer):
        timer.start("wta")
        dl, dr = wta_any(lv, D, pixel_major, out=m[0]), wta_any(rv, D, pixel_major, out=m[1])
        timer.stop()
        return dl, dr

    def _pixel_major_free(self, ws, L, R, D, left, right, sups, flag_planes, fuse, m, timer):
        """Pixel-major volumes, free-running chains (default): each volume's aggregation -> SGM -> aggregation is ONE
        chain of one-volume launches on its own stream - the left on the current stream, the right on the matcher's right
        stream; the two chains meet again only in front of the WTA-carrying last launch.  left / right: (volume, spare
        buffer); returns (dl, dr, left_volume, right_volume) - the right volume holds the result only where somebody
        reads it (views="both")."""
        hp, progs, dist = self.hp, ws["progs"], self.hp["cbca_distance"]
        n1, n2 = int(hp["cbca_num_iterations1"]), int(hp["cbca_num_iterations2"])
        if flag_planes is None and self.sgm_flags_once:      # (per-stage timing: nothing ran beside the cost volume)
            timer.start("sgm_flags")
            flag_planes = sgm_flag_planes(L, R, D, hp["sgm_D"], out=ws["sgm_flags"])
            timer.stop()
        if flag_planes is None and "scratch2" not in ws:
            ws["scratch2"] = sgm_scratch(L.shape[0], L.shape[1], D, self.device)
        chain = dict(skip_unit_regions=self.skip_unit_regions, refresh_first=self.refresh_first, timer=timer)
        main_s, right_s = torch.cuda.current_stream(), self._right_stream()
        right_s.wait_stream(main_s)
        ends = []
        for st, (v, t), sup, prog, side, scr in ((main_s, left, sups[0], progs[0], hip.MCCNN_SIDE_LEFT, ws["scratch"]),
                                                 (right_s, right, sups[1], progs[1], hip.MCCNN_SIDE_RIGHT, ws.get("scratch2"))):
            with torch.cuda.stream(st):
                # (the brackets are recorded on the chain's own stream: a stage's span beside the other chain)
                timer.span_start("aggregation_1")
                v, t = cbca_prog_chain(v, t, sup, prog, D, n1, dist, **chain)
                timer.span_stop("aggregation_1")
                timer.span_start("sgm")
                # (the flag planes of the four directions were built once, on the side stream beside the cost volume:
                # both chains read them and launch no flag kernels of their own - 8 launches of 11 us off the two
                # critical chains)
                if self.extras["sgm_independent_directions"]:
                    # (result in the former spare; the aggregation behind it starts with a launch that rewrites every
                    # pixel of its output, so it asks nothing of what the spare - now the pre-SGM volume - holds)
                    (v,), (t,) = sgm_average_independent_hwd(L, R, [v], [t], [side], D, *self._sgm_hp(), scr, timer,
                                                             flags=flag_planes)
                else:
                    sgm_average_hwd(L, R, [v], [side], D, *self._sgm_hp(), scr, timer, flags=flag_planes)
                timer.span_stop("sgm")
                timer.span_start("aggregation_2")
                v, t = cbca_prog_chain(v, t, sup, prog, D, n2 - 1 if fuse else n2, dist, total=n2, fused_last=fuse, **chain)
                timer.span_stop("aggregation_2")
                ends.append((v, t))
        main_s.wait_stream(right_s)
        (lh, lt), (rh, rt) = ends
        if not fuse:
            return self._wta(lh, rh, D, True, m, timer) + (lh, rh)
        # (the right result volume stays unwritten unless the right view's post-processing reads it)
        _prog_launch_wta((lh, lt, sups[0], progs[0]), (rh, rt, sups[1], progs[1]), D, dist, (m[0], m[1]), self.both,
                         timer)
        return m[0], m[1], lt, rt

    def _aggregate_hwd(self, progs, left, right, sups, D, n, timer, **kw):
        """One aggregation of both pixel-major volumes, joined to the current stream when it returns: the program-driven
        assembly kernel where its programs exist, cbca_hwd_kernel or - distances above CBCA_HWD_MAX_DISTANCE -
        cbca_hwd_long_kernel otherwise (same bits).  kw: wta_out / store_right."""
        (lh, lt), (rh, rt) = left, right
        if progs is None:
            return cbca_hwd_pair(lh, lt, sups[0], rh, rt, sups[1], D, int(n), self.hp["cbca_distance"], timer, **kw)
        return cbca_prog_pair(lh, lt, sups[0], rh, rt, sups[1], progs, D, int(n), self.hp["cbca_distance"], timer,
                              skip_unit_regions=self.skip_unit_regions, refresh_first=self.refresh_first,
                              right_stream=self._right_stream() if self.two_chains else None, **kw)

    def _pixel_major_joined(self, ws, L, R, D, left, right, sups, fuse, m, timer, keep):
        """Pixel-major volumes, one stage after the other on the current stream (an aggregation may fork into two chains
        inside, cbca_prog_pair): free_chains / two_chains off, shapes or distances without aggregation programs, and
        `keep`, which is handed both volumes of every stage here.  Same arguments and result as _pixel_major_free."""
        hp, progs = self.hp, ws["progs"]
        sides = [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT]
        timer.span_start("aggregation_1")
        (lh, lt), (rh, rt) = self._aggregate_hwd(progs, left, right, sups, D, hp["cbca_num_iterations1"], timer)
        timer.span_stop("aggregation_1")
        if keep is not None:
            keep["cbca1"] = (hwd_to_dhw(lh, D), hwd_to_dhw(rh, D))
        timer.span_start("sgm")
        if self.extras["sgm_independent_directions"]:
            (lh, rh), (lt, rt) = sgm_average_independent_hwd(L, R, [lh, rh], [lt, rt], sides, D, *self._sgm_hp(),
                                                             ws["scratch"], timer)
        else:
            sgm_average_hwd(L, R, [lh, rh], sides, D, *self._sgm_hp(), ws["scratch"], timer)
        timer.span_stop("sgm")
        if keep is not None:
            keep["sgm"] = (hwd_to_dhw(lh, D), hwd_to_dhw(rh, D))
        # (with the WTA in the last launch the right result volume, which nothing else reads, stays unwritten)
        timer.span_start("aggregation_2")
        (lh, lt), (rh, rt) = self._aggregate_hwd(progs, (lh, lt), (rh, rt), sups, D, hp["cbca_num_iterations2"], timer,
                                                 wta_out=(m[0], m[1]) if fuse else None,
                                                 store_right=keep is not None or self.both)
        timer.span_stop("aggregation_2")
        if keep is not None:
            keep["cbca2"] = (hwd_to_dhw(lh, D), hwd_to_dhw(rh, D))
        return ((m[0], m[1]) if fuse else self._wta(lh, rh, D, True, m, timer)) + (lh, rh)

    def _aggregate_dhw(self, left, right, sups, n, timer):
        """One aggregation of both plane-major volumes: the separable kernel takes both views in one launch; the other
        variants (reference order, two-view regions) run view by view."""
        dist, both = self.hp["cbca_distance"], self.extras["both_view_support"]
        if not both and self.cbca_order == hip.MCCNN_CBCA_SEPARABLE:
            return cbca_pair(left[0], left[1], sups[0], right[0], right[1], sups[1], n, dist, self.cbca_order, timer)
        res = []
        for (vol, tmp), own, other, side in ((left, sups[0], sups[1], hip.MCCNN_SIDE_LEFT),
                                             (right, sups[1], sups[0], hip.MCCNN_SIDE_RIGHT)):
            res.append(cbca_both_views(vol, tmp, own, other, n, dist, side, timer) if both
                       else cbca(vol, tmp, own, n, dist, self.cbca_order, timer))
        return res

    def _plane_major(self, ws, L, R, D, left, right, hwd, sups, m, timer, keep):
        """Every stage on the reference's [D,H,W] layout but SGM, which runs on pixel-major copies in the spare
        ping-pong buffers (every buffer holds either layout).  Same arguments and result as _pixel_major_free, plus the
        pixel-major views of the volume buffers."""
        hp = self.hp
        (lcv, t1d), (rcv, t2d) = self._aggregate_dhw(left, right, sups, hp["cbca_num_iterations1"], timer)
        if keep is not None:
            keep["cbca1"] = (lcv.clone(), rcv.clone())
        lh = next(h for b, h in zip(ws["vol"], hwd) if b.data_ptr() == t1d.data_ptr())
        rh = next(h for b, h in zip(ws["vol"], hwd) if b.data_ptr() == t2d.data_ptr())
        sides = [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT]
        if self.extras["sgm_independent_directions"]:
            # layout change into the spares, four passes from there into the buffers the plane-major volumes have just
            # left, change back into the spares: the volumes and their spares swap roles (no fused first pass here: it
            # composes in place)
            timer.start("dhw_to_hwd")
            dhw_to_hwd(lcv, lh)
            dhw_to_hwd(rcv, rh)
            timer.stop()
            la = next(h for b, h in zip(ws["vol"], hwd) if b.data_ptr() == lcv.data_ptr())
            ra = next(h for b, h in zip(ws["vol"], hwd) if b.data_ptr() == rcv.data_ptr())
            sgm_average_independent_hwd(L, R, [lh, rh], [la, ra], sides, D, *self._sgm_hp(), ws["scratch"], timer)
            timer.start("hwd_to_dhw")
            hwd_to_dhw(la, D, t1d)
            hwd_to_dhw(ra, D, t2d)
            timer.stop()
            lcv, t1d, rcv, t2d = t1d, lcv, t2d, rcv
        else:
            sgm_average_from_dhw(L, R, [lcv, rcv], [lh, rh], sides, D, *self._sgm_hp(), ws["scratch"], timer)
            timer.start("hwd_to_dhw")
            hwd_to_dhw(lh, D, lcv)
            hwd_to_dhw(rh, D, rcv)
            timer.stop()
        if keep is not None:
            keep["sgm"] = (lcv.clone(), rcv.clone())
        (lcv, t1d), (rcv, t2d) = self._aggregate_dhw((lcv, t1d), (rcv, t2d), sups, hp["cbca_num_iterations2"], timer)
        if keep is not None:
            keep["cbca2"] = (lcv.clone(), rcv.clone())
        return self._wta(lcv, rcv, D, False, m, timer) + (lcv, rcv)

    def _post_view(self, v, D, pixel_major, timer, keep):
        """a8 .. a11 of one view (PostView) and, in a matcher with measures, its confidence launch, on the current
        stream: the check and interpolation of `v.name`, then the view-agnostic kernels on the view's operands.  Nothing
        is allocated but what the record leaves open (None) and nothing blocks."""
        hp, ex = self.hp, self.extras
        timer.start("post" + v.suffix)
        st = lr_status(v.own, v.other, D, out=v.status, view=v.name)
        di = interpolate(v.own, st, out=v.maps[0], directions=ex["interpolation_directions"],
                         occlusion_from_left=ex["occlusion_from_left"], view=v.name)
        ds = subpixel_any(di, v.volume, D, pixel_major, out=v.maps[1], numpy1_promotion=ex["numpy1_promotion"])
        dm = median(ds, 5, 5, out=v.maps[2])
        db = bilateral(v.image, dm, 5, 5, 0, hp["blur_sigma"], hp["blur_threshold"], out=v.dst)
        timer.stop()
        stages = dict(status=st, interp=di, subpixel=ds, median=dm, bilateral=db)
        if self.confidence:
            timer.start("confidence" + v.suffix)
            stages["confidence"] = confidence_any(v.volume, D, pixel_major, v.other, self.confidence, out=v.planes,
                                                  view=v.name)
            timer.stop()
        if self.semi_dense is not None:
            # the rule on the view's final map: its own status plane and its own confidence planes
            rule, (sparse, selected, sizes, scratch) = self.semi_dense, v.semi
            timer.start("semi_dense" + v.suffix)
            stages["semi_dense"] = semi_dense(db, rule, st, stages.get("confidence"), self.confidence, out=sparse,
                                              selected=selected, sizes=sizes, scratch=scratch)
            timer.stop()
            if rule.speckle is not None:
                stages["semi_dense_selected"], stages["component_sizes"] = selected, sizes
        if keep is not None:
            keep.update((name + v.suffix, t) for name, t in stages.items())

    def _check_given(self, t, shape, name, dims, like, both=None):
        """Refuses a caller's `out` / `confidence_out` that the last kernel of a view could not write."""
        both = self.both if both is None else both
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != like.device):
            raise ValueError("match: %s`%s` must be a contiguous float32 [%s%s] tensor on the images' device" % (
                "with views='both' " if both else "", name, "2," if both else "", dims))

    @staticmethod
    def _hand_out(t, given, handed):
        """The hand-out rule of every result.  The workspace tensor is overwritten by the next pair: the caller gets a copy
        unless the tensor is its own (`given`) or `handed`: a fresh one (keep=) or the static buffer (match_graph)."""
        return t if (handed or given is not None) else t.clone()

    def _match(self, left_image, right_image, ndisp, given=PairResult(None), timer=_NO_TIMER, keep=None, _static_out=False):
        """left/right: standardised float32 device tensors [H,W] (or [H,W,1]).  Returns the PairResult of the pair: the
        final left disparity map [H,W] on the device, the planes of a matcher with confidence measures and the sparse map
        of one with a semi-dense rule.  The matcher's workspace is reused by the next call, so the map is handed out as a
        copy - one [H,W] allocation + one copy per pair; with the caller's `out` in given.map (a contiguous float32 [H,W]
        device tensor) the last kernel writes there instead: nothing is allocated but the conv activations; the other
        fields follow the same rule.  `keep`, if a dict, receives intermediate device tensors in the reference's [D,H,W]
        layout (tests)."""
        L = left_image.reshape(left_image.shape[0], left_image.shape[1]).contiguous()
        R = right_image.reshape(right_image.shape[0], right_image.shape[1]).contiguous()
        H, W = L.shape
        D = int(ndisp)
        ws = self.workspace(H, W, D)
        dp = hwd_pitch(D)
        dhw = [b[:D * H * W].view(D, H, W) for b in ws["vol"]]      # every volume buffer in either layout
        hwd = [b[:H * W * dp].view(H, W, dp) for b in ws["vol"]]
        # Without per-stage timing the side work runs beside the cost volume; with it, on the main stream behind it.
        overlap = timer is _NO_TIMER
        # Free-running chains need the one-volume program launches (program buffers exist on the pixel-major "prog"
        # route only); with `keep` the stages are joined, so that both volumes of a stage can be handed out.
        free = self.free_chains and self.two_chains and keep is None and ws["progs"] is not None
        flag_planes = None

        timer.start("features")
        if self.features == "split_f16":
            fl, fr = self.net.features_pair_hwc_split(L, R)
        else:
            fl, fr = self.net.features_pair_hwc(L, R, tile_rows=self.feature_tile_rows)
        timer.stop()
        if overlap:
            sup_l, sup_r, flag_planes, ready = self._side_work(ws, L, R, D, want_flags=free and self.sgm_flags_once)
        lv, rv, pixel_major = self._cost_volumes(fl, fr, D, dhw, hwd, timer, ws)
        del fl, fr
        if keep is not None:
            keep["cv"] = (hwd_to_dhw(lv, D), hwd_to_dhw(rv, D)) if pixel_major else (lv.clone(), rv.clone())
        if overlap:
            torch.cuda.current_stream().wait_event(ready)
        else:
            sup_l, sup_r = self._side_work_timed(ws, L, R, D, timer)
        sups = (sup_l, sup_r)

        m = ws["maps"] if keep is None else torch.empty_like(ws["maps"])
        if self.pixel_major():
            if not pixel_major:
                timer.start("cv_to_pixel_major")
                lv, rv = dhw_to_hwd(lv, hwd[2]), dhw_to_hwd(rv, hwd[3])
                timer.stop()
            # The second aggregation's last iteration carries the WTA of both results when a wave holds all disparities
            # of a pixel and the arms are short enough for the kernels that have that form (on the free path the
            # program buffers imply the distance term).
            fuse = (int(self.hp["cbca_num_iterations2"]) >= 1 and D <= cbca_hwd_wta_max_d()
                    and int(self.hp["cbca_distance"]) <= CBCA_HWD_MAX_DISTANCE)
            if free:
                dl, dr, left_volume, right_volume = self._pixel_major_free(ws, L, R, D, (lv, hwd[0]), (rv, hwd[1]), sups,
                                                                           flag_planes, fuse, m, timer)
            else:
                dl, dr, left_volume, right_volume = self._pixel_major_joined(ws, L, R, D, (lv, hwd[0]), (rv, hwd[1]), sups,
                                                                             fuse, m, timer, keep)
        else:
            dl, dr, left_volume, right_volume = self._plane_major(ws, L, R, D, (lv, dhw[2]), (rv, dhw[3]), hwd, sups, m,
                                                                  timer, keep)

        # a8 .. a11 and the confidence planes, view by view.  Per-pair maps live in the workspace unless the caller keeps
        # intermediates (tests: fresh tensors then): apart from the returned map (see `out`) a pair allocates nothing but
        # the conv activations and never blocks the host.  views="both": one [2,H,W] tensor (and [2,K,H,W] planes) takes
        # the two views' results.
        both, k, fresh, pm = self.both, len(self.confidence), keep is not None, self.pixel_major()
        lead, semi = (2,) if both else (), self.semi_dense is not None

        def dest(given, spare):         # the caller's tensor, else the workspace's - under keep= a fresh one like it
            return given if given is not None else (torch.empty_like(spare) if fresh else spare)
        # per result: the caller's keyword, the workspace's tensor (None: this matcher has no such result), the shape, and
        # the shape as a refusal words it.  (A left-only matcher without measures never looks at confidence_out.)
        rows = (("out", ws["both"] if both else ws["maps"][5], (H, W), "H,W"),
                ("confidence_out", ws["confidence"] if k else None, (k, H, W), "K,H,W"),
                ("semi_out", ws["sparse"] if semi else None, (H, W), "H,W"))
        res = []
        for t, (name, spare, shape, dims) in zip(given, rows):
            if spare is not None or (both and name == "confidence_out"):
                self._check_given(t, lead + shape, name, dims, L)
            res.append(dest(t, spare) if spare is not None else None)
        # the metric outputs: the left view's, no leading axis (no keyword hands in the number of points: the workspace's,
        # or a replayed graph's static word when its pair is repeated)
        geo = self.geometry
        if geo is not None:
            if geo["calib"] is None:
                raise ValueError("match: geometry= without a calibration (geometry=dict(calib=...) or set_calibration())")
            for t, name, key, shape, dims in ((given.depth, "depth_out", "depth", (H, W), "H,W"),
                                              (given.points, "points_out", "points", (H * W, 4), "H*W,4")):
                if geo[key]:
                    self._check_given(t, shape, name, dims, L, both=False)
                res.append(dest(t, ws[key]) if geo[key] else None)
            res.append(dest(given.n_points, ws["n_points"]) if geo["points"] else None)
        res = PairResult(*res)
        if semi:
            # the selection and the size plane, one [H,W] per view, and each view's labelling scratch
            selected, sizes = (dest(None, ws[key]).view(-1, H, W) for key in ("semi_selected", "semi_sizes"))
            scratch = [torch.empty_like(t) for t in ws["semi_scratch"]] if fresh else ws["semi_scratch"]

        def results_of(i):              # where view i's results go (PostView's dst, planes and semi)
            r = res.view(i, both)
            return dict(dst=r.map, planes=r.planes, semi=(r.sparse, selected[i], sizes[i], scratch[i]) if semi else None)
        main_s = torch.cuda.current_stream()
        fork = both and timer is _NO_TIMER
        if both:
            # The right view first: without per-stage timing its launches are queued on the matcher's right stream, forked
            # from the current one here, and run beside the left view's, which follow on the current one; the two join in
            # front of nothing but the hand-out.  Under per-stage timing everything stays on the current stream.
            right_s = self._right_stream() if fork else main_s
            if fork:
                right_s.wait_stream(main_s)
            view = PostView("right", "_right", R, dr, dl, right_volume, None if fresh else ws["status_right"],
                            torch.empty_like(ws["maps_right"]) if fresh else ws["maps_right"], stream=right_s,
                            **results_of(1))
            with torch.cuda.stream(view.stream):
                self._post_view(view, D, pm, timer, keep)
            if fresh:
                keep["cbca2_right"] = hwd_to_dhw(right_volume, D) if pm else right_volume.clone()
        view = PostView("left", "", L, dl, dr, left_volume, None if fresh else ws["status"], m[2:5], stream=main_s,
                        **results_of(0))
        self._post_view(view, D, pm, timer, keep)
        if geo is not None:
            # behind the left view's post-processing and semi-dense stage, on the pair's stream: the depth of the dense
            # map, the cloud of the sparse map where there is one
            left = res.view(0, both)
            timer.start("geometry")
            if geo["depth"]:
                depth(left.map, geo["calib"], out=res.depth)
            if geo["points"]:
                reproject(left.sparse if semi else left.map, geo["calib"], geo["max_depth"], out=res.points,
                          n_out=res.n_points, scratch=torch.empty_like(ws["points_scratch"]) if fresh else ws["points_scratch"])
            timer.stop()
            if fresh:
                keep.update((k, t) for k, t in (("depth", res.depth), ("points", res.points), ("n_points", res.n_points))
                            if t is not None)
        if fork:
            main_s.wait_stream(right_s)
        if fresh:
            keep["wta"] = (dl, dr)
        handed = _static_out or fresh
        return PairResult(*(self._hand_out(t, g, handed) if t is not None else None for t, g in zip(res, given)))

    def _ingest_buffers(self, H, W):
        """Static float32 inputs + ingest scratch of the eager byte path: kept per shape, so that a pair allocates
        nothing (the workspace is reused by the next pair in the same way)."""
        b = self._ingest
        if b is None or b[0] != (H, W):
            dev = self.device
            b = ((H, W), torch.empty((H, W), dtype=torch.float32, device=dev),
                 torch.empty((H, W), dtype=torch.float32, device=dev), ingest_scratch(H, W, dev))
            self._ingest = b
        return b[1:]

    def match_u8(self, left_u8, right_u8, ndisp, out=None, confidence_out=None, semi_out=None, depth_out=None,
                 points_out=None):
        """match() straight from the decoded bytes of the two PNGs: uint8 device tensors [H,W] or [H,W,C] (C = 1, 3, 4;
        see ingest_u8), or pinned host tensors, which are copied in stream order without blocking.  The standardisation runs on the device, bit-identical to match.py's on the host, so the map is
        what match() returns on the host-standardised images."""
        H, W, _ = _u8_image(left_u8)
        sl, sr, scratch = self._ingest_buffers(H, W)
        left_u8 = left_u8.to(self.device, non_blocking=True).contiguous()
        right_u8 = right_u8.to(self.device, non_blocking=True).contiguous()
        ingest_u8_pair(left_u8, right_u8, sl, sr, scratch)
        return self.match(sl, sr, ndisp, out=out, confidence_out=confidence_out, semi_out=semi_out, depth_out=depth_out,
                          points_out=points_out)

    def _graph_key(self, key):
        """The key of a pair's captured graph.  An accurate network's graph holds the ADDRESS of the packed decision
        operands and the final bias by value (ACCURATE_NET.decision_operands rebuilds both when a weight tensor changes),
        so its key carries the network's decision_weights_key(): after an optimiser step or a load_state the pair is
        captured again, and the graphs of the weights before are dropped (a replay of one would read the earlier
        weights' buffer, or memory the allocator has handed on).  The tower's weights are read in place and need none."""
        if self.geometry is not None:
            # the calibration and max_depth are launch arguments held by value: one graph per calibration of a shape
            calib = self.geometry["calib"]
            key = key + (("geometry", calib.scalars() if calib is not None else None, _f32(self.geometry["max_depth"])),)
        if not self.accurate:
            return key
        key = key + (self.net.decision_weights_key(),)
        for k in [k for k in self._graphs if k[-1] != key[-1]]:
            del self._graphs[k]
        return key

    def _capture(self, key, shape, make_static, prologue=None):
        """One pair captured as a graph: self._graphs[key] = (graph, static, out).  make_static() allocates and fills
        the static inputs - static[0], static[1]: the float32 images the pair reads - once the workspace is resident;
        prologue(*static), if given, is issued in front of every pair, inside the graph too (the ingest launches).
        The order is the rule:
          1. workspace() before anything else - it may reset self._graphs (one shape resident at a time);
          2. fresh side / right-chain streams for this capture: a stream never takes part in the captures of two graphs
             (see _right_stream);
          3. two eager warm-up pairs on a stream of their own, so that MIOpen has chosen its kernels and the allocator
             its blocks, joined to the current stream;
          4. every stream the pair touches (the side stream of the builder, the right volume's chain) idle before the
             capture begins: streams that enter a capture with eager work still queued have crashed the runtime once."""
        H, W, D = shape
        self.workspace(H, W, D)
        self._side = self._right = None
        static = make_static()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                if prologue is not None:
                    prologue(*static)
                self._match(static[0], static[1], D)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            if prologue is not None:
                prologue(*static)
            out = self._match(static[0], static[1], D, _static_out=True).public()
        self._graphs[key] = (graph, static, out)
        return self._graphs[key]

    def _saturated_graph_pair(self, sl, sr, ndisp, out):
        """on_saturation behind a replay (one host synchronisation unless "ignore"): a repeated pair writes the static
        map - and the static confidence planes and sparse map, where the matcher produces them."""
        self._saturated_pair(sl, sr, ndisp, self.result_of(out))

    def _static_u8(self, left_u8, right_u8, H, W):
        """The static buffers of match_graph_u8: (float32 left, right, the byte images, the ingest scratch)."""
        bl = torch.empty(tuple(left_u8.shape), dtype=torch.uint8, device=self.device)
        br = torch.empty_like(bl)
        sl = torch.empty((H, W), dtype=torch.float32, device=self.device)
        sr = torch.empty((H, W), dtype=torch.float32, device=self.device)
        scratch = ingest_scratch(H, W, self.device)
        bl.copy_(left_u8)
        br.copy_(right_u8)
        return sl, sr, bl, br, scratch

    def match_graph_u8(self, left_u8, right_u8, ndisp):
        """match_graph() from bytes: static uint8 inputs, and the ingest launches INSIDE the captured graph, writing the
        static float32 images the rest of the graph reads - per pair two byte copies (from the device or from pinned host
        memory, in stream order, non-blocking) and one replay.  One graph per (H, W, ndisp, C), captured by the rules of
        _capture.  Returns the static output map (overwritten by the next call) - what match_graph() returns: with
        confidence measures and / or a semi-dense rule the tuple (map[, planes][, sparse]), every element static."""
        H, W, C = _u8_image(left_u8)
        if _u8_image(right_u8) != (H, W, C):
            raise ValueError("match_graph_u8: the two images must have the same shape")
        key = self._graph_key((H, W, int(ndisp), "u8", C))
        g = self._graphs.get(key) or self._capture(
            key, key[:3], lambda: self._static_u8(left_u8, right_u8, H, W),
            lambda sl, sr, bl, br, scratch: ingest_u8_pair(bl, br, sl, sr, scratch))
        graph, (sl, sr, bl, br, _scratch), out = g
        bl.copy_(left_u8, non_blocking=True)
        br.copy_(right_u8, non_blocking=True)
        graph.replay()
        self._saturated_graph_pair(sl, sr, ndisp, out)
        return out

    @staticmethod
    def _static_f32(L, R):
        sl, sr = torch.empty_like(L, dtype=torch.float32), torch.empty_like(R, dtype=torch.float32)
        sl.copy_(L)
        sr.copy_(R)
        return sl, sr

    def match_graph(self, left_image, right_image, ndisp):
        """match() replayed as ONE hipGraph launch: the ~75 kernel launches of a pair are captured once per image
        shape (_capture) and replayed on static input/output buffers.  Returns the static output map [H,W] (overwritten
        by the next call; with confidence measures (map, planes), with a semi-dense rule the sparse map as the last element
        besides - (map, sparse) or (map, planes, sparse) - all static).  The images are copied into the static inputs in stream order; nothing synchronises."""
        L = left_image.reshape(left_image.shape[0], left_image.shape[1])
        R = right_image.reshape(right_image.shape[0], right_image.shape[1])
        key = self._graph_key((L.shape[0], L.shape[1], int(ndisp)))
        graph, (sl, sr), out = self._graphs.get(key) or self._capture(key, key[:3], lambda: self._static_f32(L, R))
        sl.copy_(L)
        sr.copy_(R)
        graph.replay()
        self._saturated_graph_pair(sl, sr, ndisp, out)
        return out


class SaturationRedo(object):
    """The repeat policy of a list loop whose matchers run with on_saturation="ignore" (several pairs in flight share
    one flag).  The hand-written kernels report an activation beyond the range of their stored records (never seen on
    standardised images with the trained weights): that pair - and, with several in flight, the ones that shared the
    flag with it - is matched again by a library matcher, built when the first pair needs it.

    matchers: one per pair in flight (they share the network, and with it the flag: the first is asked);
    make_library_matcher(): the matcher that repeats a pair."""

    def __init__(self, matchers, make_library_matcher):
        self.matchers, self.make_library_matcher = matchers, make_library_matcher
        self.left = 0                # pairs still to repeat: this one and the next len(matchers) - 1
        self._matcher = None

    def due(self):
        """Asked once per pair, in list order, when the pair's map is complete: True when it is to be repeated.
        Reads the flag (which blocks the host) only where the last pair ran a kernel that raises it."""
        m0 = self.matchers[0]
        if m0.saturation_checked() and m0.features_saturated():
            self.left = len(self.matchers)
        if self.left <= 0:
            return False
        self.left -= 1
        return True

    def matcher(self):
        if self._matcher is None:
            self._matcher = self.make_library_matcher()
        return self._matcher

    def notice(self, path):
        """What a loop prints when it repeats the pair whose map is `path`."""
        return self.matchers[0].saturation_notice().format(path)
