"""Drop-in for /root/reference/src/process_functional.py: the same eleven functions, same argument order, same
return values, computed on an MI355X through libmccnn_hip.so (include/mccnn.h).

    from process_functional import *          # exactly what the reference's match.py:13 does

Arrays may be NumPy (the reference's convention: float32, images [H,W,1], features [H,W,64], volumes [D,H,W],
maps [H,W]) or torch device tensors; the result comes back in the kind that went in.  NumPy inputs are copied to
HBM, processed, and copied back - use stereo_device.StereoMatcher to keep a whole pair resident instead.

There is no CPU fallback: without a HIP device or without the built library every function raises.

Options the reference does not have (module attributes; the DEFAULTS are the bit-exact variants, so that a drop-in
user gets the reference's numbers - the fast ones are opt-in and only tolerance-bounded):
    COST_VOLUME_MODE  "exact" (NumPy summation order, bit-exact, default) | "mfma" (matrix cores, <= 2e-6 abs)
    CBCA_ORDER        "reference" (flat list order, bit-exact, default: the pixel-major kernels - mccnn_cbca_iter_hwd
                        and the aggregation programs up to distance 14, mccnn_cbca_iter_hwd_long for 15 to 32)
                      | "reference_plane_major" (the same sums by the plane-major kernel of mccnn_cbca_iter - slower)
                      | "separable" (fast, <= 1e-6 abs per iteration)
Opt-in departures from the reference's results (defaults reproduce it):
    CBCA_BOTH_VIEWS          False | True  - the paper's support regions intersected with the other view's (pf:122-144
                                             names it and skips it as impractical; pf:661-729 is its dead attempt)
    INTERPOLATION_DIRECTIONS 4 | 16        - mismatches filled from 16 rays as in the paper (pf:318)
    OCCLUSION_FROM_LEFT      False | True  - occlusions filled from the nearest match on the left, as in the paper (pf:361)
    SGM_INDEPENDENT_DIRECTIONS False | True - SGM_average as the paper defines it and pf:195-210 spells it: the four
                                             directions each computed from the SAME input volume and averaged,
                                             (((right + left) + up) + bottom) / 4. in float32.  The reference composes
                                             the four passes on one aliased array (semi_global_matching returns its
                                             argument) and its average is the identity; that stays the default.  With
                                             the switch on SGM_average leaves its arguments unmodified.
    VERTICAL_RANGE           0 | 1 .. 4    - compute_cost_volume for imperfectly rectified pairs: every pixel keeps, per
                                             disparity, its best score over the other view's rows h - R .. h + R
                                             (include/mccnn.h: mccnn_cost_volume_vertical_hwd; "exact" mode, ndisp <= 1024)
    VERTICAL_OFFSET          0 | -8 .. 8   - compute_cost_volume along a row offset: the volumes against row h + offset of
                                             the other view, VERTICAL_RANGE searched around it (include/mccnn.h:
                                             mccnn_cost_volume_offset_hwd; "exact" mode); vertical_profile() measures it
                             | "grid"      - ... along a field of offsets, one per cell of VERTICAL_OFFSET_GRID = (gh, gw)
                                             cells (clamped per shape), measured from the pair's own features at
                                             VERTICAL_OFFSET_PROFILE = (max_offset, row_step) (include/mccnn.h:
                                             mccnn_vertical_field_select, mccnn_cost_volume_field_hwd)
    NUMPY1_PROMOTION         False | True  - sub-pixel formula evaluated as NumPy < 2 promotes its scalars (float64,
                                             rounded once): what the reference's own Python 2.7 + NumPy 1.14 computes;
                                             the default is NumPy >= 2's float32 chain, which the golden vectors pin
"""
import hashlib

import numpy as np
import torch

import _hipabi as hip
import stereo_device as sd
from model import ACCURATE_NET, NET

FEATURES = "split_f16"       # "split_f16": hand-written matrix-core conv stack (float32-accurate); "library": MIOpen
COST_VOLUME_MODE = "exact"
ACCURATE_DECISION = "auto"   # compute_cost_volume_accurate: "auto" | "kernel" (csrc/decision_mfma.hip) | "library" (torch)
CBCA_ORDER = "reference"
CBCA_BOTH_VIEWS = False
INTERPOLATION_DIRECTIONS = 4
OCCLUSION_FROM_LEFT = False
NUMPY1_PROMOTION = False
SGM_INDEPENDENT_DIRECTIONS = False
VERTICAL_RANGE = 0
VERTICAL_OFFSET = 0
VERTICAL_OFFSET_GRID = (3, 4)
VERTICAL_OFFSET_PROFILE = (4, 8)

_CV_MODES = {"exact": hip.MCCNN_CV_EXACT, "mfma": hip.MCCNN_CV_MFMA}
_CBCA_ORDERS = {"separable": hip.MCCNN_CBCA_SEPARABLE, "reference": hip.MCCNN_CBCA_REFERENCE_ORDER,
                "reference_plane_major": hip.MCCNN_CBCA_REFERENCE_ORDER}

__all__ = ["compute_features", "compute_cost_volume", "compute_cost_volume_accurate", "cost_volume_aggregation", "SGM_average",
           "disparity_prediction", "interpolation", "subpixel_enhance", "median_filter", "bilateral_filter",
           "semi_global_matching", "compute_cross_region", "confidence_measures", "interpolation_right", "semi_dense",
           "speckle_filter", "vertical_profile", "depth_from_disparity", "reproject"]


def _dev(x, dtype=torch.float32):
    """-> (contiguous device tensor, came_from_numpy)"""
    device = hip.require_device()
    if torch.is_tensor(x):
        return x.to(device=device, dtype=dtype).contiguous(), False
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device), True


def _img(x):
    t, was_np = _dev(x)
    if t.dim() == 3:
        assert t.shape[2] == 1, "images are [H,W,1] (match.py:122-125)"
        t = t.reshape(t.shape[0], t.shape[1])
    return t.contiguous(), was_np


def _ret(t, was_np):
    return t.cpu().numpy() if was_np else t


_NET_CACHE = {}


def _net_for(checkpoint, patch_height):
    key = (checkpoint, patch_height)
    net = _NET_CACHE.get(key)
    if net is None:
        device = hip.require_device()
        net = NET(None, input_patch_size=patch_height, num_conv_layers=(patch_height - 1) // 2, batch_size=1,
                  device=device)
        net.restore(checkpoint)  # raises for None, like Saver.restore(sess, None) does (pf:43)
        _NET_CACHE.clear()
        _NET_CACHE[key] = net
    return net


def compute_features(left_image, right_image, patch_height, patch_width, checkpoint):
    """pf:15-73.  The weights stay resident between calls (the reference rebuilds graph + session per pair)."""
    assert patch_height == patch_width, "square patches only (match.py:61-62)"
    L, was_np = _img(left_image)
    R, _ = _img(right_image)
    net = checkpoint if isinstance(checkpoint, NET) else _net_for(checkpoint, patch_height)
    if FEATURES == "split_f16" and net.supports_split_features():
        # the hand-written matrix-core stack (float32-accurate; csrc/conv_mfma.hip); should an activation leave the
        # range of its stored records, the float32 library convolutions take the pair instead
        fl, fr = net.features_pair_hwc_split(L, R)
        if not net.split_saturated():
            return _ret(fl, was_np), _ret(fr, was_np)
    return _ret(net.features_hwc(L), was_np), _ret(net.features_hwc(R), was_np)


def compute_cost_volume(featuresl, featuresr, ndisp):
    """pf:78-113."""
    fl, was_np = _dev(featuresl)
    fr, _ = _dev(featuresr)
    if VERTICAL_OFFSET == "grid":
        if COST_VOLUME_MODE != "exact":
            raise ValueError("VERTICAL_OFFSET='grid': the row offset exists for COST_VOLUME_MODE 'exact' only")
        R, step = (int(v) for v in VERTICAL_OFFSET_PROFILE)
        grid = sd.vertical_field_grid(fl.shape[0], fl.shape[1], VERTICAL_OFFSET_GRID, step)
        votes = sd.vertical_profile(fl, fr, int(ndisp), R, step)
        field = sd.vertical_field_select(votes, fl.shape[0], step, R, grid)[0]
        hl, hr = sd.cost_volume_field_hwd(fl, fr, int(ndisp), field, VERTICAL_RANGE)
        return _ret(sd.hwd_to_dhw(hl, int(ndisp)), was_np), _ret(sd.hwd_to_dhw(hr, int(ndisp)), was_np)
    if VERTICAL_OFFSET:
        if isinstance(VERTICAL_OFFSET, bool) or not isinstance(VERTICAL_OFFSET, int) \
                or abs(VERTICAL_OFFSET) > sd.VERTICAL_OFFSET_MAX:
            raise ValueError("VERTICAL_OFFSET=%r: an integer in [-%d, %d]" % (VERTICAL_OFFSET, sd.VERTICAL_OFFSET_MAX,
                                                                            sd.VERTICAL_OFFSET_MAX))
        if COST_VOLUME_MODE != "exact":
            raise ValueError("VERTICAL_OFFSET=%r: the row offset exists for COST_VOLUME_MODE 'exact' only" % VERTICAL_OFFSET)
        k0 = torch.tensor([VERTICAL_OFFSET], dtype=torch.int32, device=fl.device)
        hl, hr = sd.cost_volume_offset_hwd(fl, fr, int(ndisp), k0, VERTICAL_RANGE)
        return _ret(sd.hwd_to_dhw(hl, int(ndisp)), was_np), _ret(sd.hwd_to_dhw(hr, int(ndisp)), was_np)
    if VERTICAL_RANGE:
        if COST_VOLUME_MODE != "exact":
            raise ValueError("VERTICAL_RANGE=%r: the vertical search exists for COST_VOLUME_MODE 'exact' only" % VERTICAL_RANGE)
        hl, hr = sd.cost_volume_vertical_hwd(fl, fr, int(ndisp), VERTICAL_RANGE)
        return _ret(sd.hwd_to_dhw(hl, int(ndisp)), was_np), _ret(sd.hwd_to_dhw(hr, int(ndisp)), was_np)
    lcv, rcv = sd.cost_volume(fl, fr, int(ndisp), _CV_MODES[COST_VOLUME_MODE])
    return _ret(lcv, was_np), _ret(rcv, was_np)


def vertical_profile(featuresl, featuresr, ndisp, max_offset, row_step):
    """The row offset of a pair, measured from its features (include/mccnn.h: mccnn_vertical_profile and
    mccnn_vertical_offset_select): NumPy in, (offset int, totals uint64 [2 max_offset + 1], votes uint32 [n_rows,
    ceil(W / 64), 2 max_offset + 1]) out."""
    fl, _ = _dev(featuresl)
    fr, _ = _dev(featuresr)
    votes = sd.vertical_profile(fl, fr, int(ndisp), int(max_offset), int(row_step))
    offset, totals = sd.vertical_offset_select(votes, int(max_offset))
    return (int(offset.cpu().numpy()[0]), totals.cpu().numpy().view(np.uint64), votes.cpu().numpy().view(np.uint32))


_DECISION_NETS = {}


def compute_cost_volume_accurate(featuresl, featuresr, ndisp, fc_layers):
    """The accurate network's counterpart of compute_cost_volume (no such function in the reference, whose README
    leaves the architecture out): features [H,W,C] as compute_features returns them for an ACCURATE_NET, fc_layers
    that network itself or its checkpoint's list of (weights [in,out], biases) pairs fc1 .. fc<n+1>.  Returns
    (lcv, rcv) [D,H,W] = -sigmoid score, borders as compute_cost_volume.  COST_VOLUME_MODE "exact" selects the
    float32-accurate split-operand kernel, "mfma" the plain f16 one; ACCURATE_DECISION the route."""
    import warnings
    fl, was_np = _dev(featuresl)
    fr, _ = _dev(featuresr)
    if isinstance(fc_layers, ACCURATE_NET):
        net = fc_layers
    else:
        # keyed on the CONTENT of the arrays (the network holds copies of them): an array edited in place, or a new one
        # at a recycled address, gets its own packed weights
        digest = hashlib.sha1()
        for w, b in fc_layers:
            for a in (w, b):
                a = np.ascontiguousarray(a, dtype=np.float32)
                digest.update(repr(a.shape).encode())
                digest.update(a.tobytes())
        key = (digest.hexdigest(), int(fl.shape[-1]), str(fl.device))
        net = _DECISION_NETS.get(key)
        if net is None:
            net = ACCURATE_NET(None, num_conv_layers=0, num_conv_feature_maps=int(fl.shape[-1]), batch_size=1,
                               device=fl.device, num_fc_layers=len(fc_layers) - 1,
                               num_fc_units=int(np.shape(fc_layers[0][0])[1]))
            net.set_layers([], fc_layers)
            _DECISION_NETS.clear()
            _DECISION_NETS[key] = net
    route = ACCURATE_DECISION
    if route != "library":
        why = sd.decision_kernel_refusal(net, int(fl.shape[1]), int(ndisp))
        if why is not None and route == "kernel":
            raise ValueError("ACCURATE_DECISION='kernel': %s" % why)
        if why is not None:
            warnings.warn("accurate network: %s; the decision stage runs on the float32 library route" % why)
        route = "library" if why is not None else (sd.DECISION_AUTO if route == "auto" else "kernel")
    lcv, rcv = sd.cost_volume_accurate(net, fl, fr, int(ndisp), _CV_MODES[COST_VOLUME_MODE], decision=route,
                                       pixel_major=False)
    return _ret(lcv, was_np), _ret(rcv, was_np)


def compute_cross_region(image, intensity_threshold, distance_threshold):
    """pf:571-657: (union_region int32 [H,W,(2L)^2,2] padded with -1, union_region_num int32 [H,W]).
    Only for API compatibility / small images - the aggregation below never materialises the lists."""
    img, was_np = _img(image)
    support = sd.cross_arms(img, intensity_threshold, int(distance_threshold))
    region = sd.cross_region_list(support, int(distance_threshold))
    return _ret(region, was_np), _ret(sd.support_count(support).contiguous(), was_np)


def cost_volume_aggregation(left_image, right_image, left_cost_volume, right_cost_volume,
                            intensity_threshold, distance_threshold, max_average_time):
    """pf:117-183.  Inputs are not modified; fresh volumes are returned."""
    outs = []
    was_np = False
    images = [_img(left_image)[0], _img(right_image)[0]]
    supports = [sd.cross_arms(img, intensity_threshold, int(distance_threshold)) for img in images]
    pixel_major = not CBCA_BOTH_VIEWS and CBCA_ORDER == "reference" and sd.aggregation_route(
        distance_threshold, images[0].shape[1], 1, _CBCA_ORDERS[CBCA_ORDER]) != "plane_major"
    if pixel_major and int(distance_threshold) <= sd.CBCA_HWD_MAX_DISTANCE:
        # What match.py's default runs: the reference's summation order on pixel-major copies, both views per launch,
        # through the program-driven assembly kernel (its programs are built once here and serve every iteration; from
        # the second iteration on the pixels whose support region is the pixel itself are left alone - same bits).
        vl, was_np = _dev(left_cost_volume)
        vr, _ = _dev(right_cost_volume)
        D, H, W = vl.shape
        progs = sd.cbca_prog_buffers(D, H, W, vl.device) if tuple(vr.shape) == (D, H, W) else None
        if progs is not None:
            sd.cbca_prog_build_pair(supports[0], supports[1], D, int(distance_threshold), progs,
                                    "both" if int(max_average_time) >= 2 else "full")
            hl, hr = sd.dhw_to_hwd(vl), sd.dhw_to_hwd(vr)       # copies: the caller's arrays stay as they are
            (rl, _), (rr, _) = sd.cbca_prog_pair(hl, torch.empty_like(hl), supports[0], hr, torch.empty_like(hr),
                                                 supports[1], progs, D, int(max_average_time), int(distance_threshold),
                                                 right_stream=sd.right_stream(hl.device))
            return _ret(sd.hwd_to_dhw(rl, D), was_np), _ret(sd.hwd_to_dhw(rr, D), was_np)
    for k, vol in enumerate((left_cost_volume, right_cost_volume)):
        v, was_np = _dev(vol)
        if torch.is_tensor(vol) and v.data_ptr() == vol.data_ptr():
            v = v.clone()  # the ping-pong clobbers its input; the reference leaves the caller's array alone
        if CBCA_BOTH_VIEWS:
            res, _spare = sd.cbca_both_views(v, torch.empty_like(v), supports[k], supports[1 - k], int(max_average_time),
                                             int(distance_threshold), hip.MCCNN_SIDE_LEFT if k == 0 else hip.MCCNN_SIDE_RIGHT)
        elif pixel_major:
            # the reference's summation order on a pixel-major copy (disparities on lanes; sd.cbca_hwd picks the kernel
            # by distance): bit-identical to the plane-major reference-order kernel, several times faster
            D = v.shape[0]
            hv = sd.dhw_to_hwd(v)
            hres, _spare = sd.cbca_hwd(hv, torch.empty_like(hv), supports[k], D, int(max_average_time),
                                       int(distance_threshold))
            res = sd.hwd_to_dhw(hres, D)
        else:
            res, _spare = sd.cbca(v, torch.empty_like(v), supports[k], int(max_average_time), int(distance_threshold),
                                  _CBCA_ORDERS[CBCA_ORDER])
        outs.append(_ret(res, was_np))
    return outs[0], outs[1]


def semi_global_matching(left_image, right_image, cost_volume, r, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, choice):
    """pf:476-568.  Updates `cost_volume` IN PLACE and returns it, as the reference does (pf:544,568)."""
    assert choice == "R" or choice == "L"
    rh, rw = int(r[0]), int(r[1])
    assert rh * rw == 0
    L, _ = _img(left_image)
    R, _ = _img(right_image)
    v, was_np = _dev(cost_volume)
    D, H, W = v.shape
    hwd = sd.dhw_to_hwd(v)
    scratch = sd.sgm_scratch(H, W, D, v.device)
    f32 = sd._f32
    sd.sgm_pass_hwd(L, R, [hwd], [hip.MCCNN_SIDE_LEFT if choice == "L" else hip.MCCNN_SIDE_RIGHT], D, (rh, rw),
                    f32(sgm_P1), f32(sgm_P2), f32(sgm_Q1), f32(sgm_Q2), f32(sgm_D), scratch)
    sd.hwd_to_dhw(hwd, D, v)
    if was_np:
        cost_volume[...] = v.cpu().numpy()
    elif v.data_ptr() != cost_volume.data_ptr():
        cost_volume.copy_(v)
    return cost_volume


def SGM_average(left_cost_volume, right_cost_volume, left_image, right_image,
                sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V):
    """pf:187-235.  Like the reference, the two volume arguments end up holding the result as well (its four
    semi_global_matching calls run in place on them) and new arrays are returned.  SGM_INDEPENDENT_DIRECTIONS: the
    paper's average of four independent directions instead, and the arguments are left as they are."""
    L, _ = _img(left_image)
    R, _ = _img(right_image)
    vl, was_np = _dev(left_cost_volume)
    vr, _ = _dev(right_cost_volume)
    D, H, W = vl.shape
    hwd_shape = (H, W, sd.hwd_pitch(D))
    hl = torch.empty(hwd_shape, dtype=torch.float32, device=vl.device)
    hr = torch.empty(hwd_shape, dtype=torch.float32, device=vl.device)
    scratch = sd.sgm_scratch(H, W, D, vl.device)
    if SGM_INDEPENDENT_DIRECTIONS:
        # the four directions from the same volume, averaged: out of place, the arguments keep their values
        sl, sr = sd.dhw_to_hwd(vl), sd.dhw_to_hwd(vr)
        sd.sgm_average_independent_hwd(L, R, [sl, sr], [hl, hr], [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT], D, sgm_P1,
                                       sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V, scratch)
        ol, orr = sd.hwd_to_dhw(hl, D), sd.hwd_to_dhw(hr, D)
        return (ol.cpu().numpy(), orr.cpu().numpy()) if was_np else (ol, orr)
    sd.sgm_average_from_dhw(L, R, [vl, vr], [hl, hr], [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT], D, sgm_P1, sgm_P2,
                            sgm_Q1, sgm_Q2, sgm_D, sgm_V, scratch)
    ol, orr = sd.hwd_to_dhw(hl, D), sd.hwd_to_dhw(hr, D)
    if was_np:
        ol_np, or_np = ol.cpu().numpy(), orr.cpu().numpy()
        left_cost_volume[...] = ol_np
        right_cost_volume[...] = or_np
        return ol_np.copy(), or_np.copy()
    left_cost_volume.copy_(ol)
    right_cost_volume.copy_(orr)
    return ol, orr


def disparity_prediction(left_cost_volume, right_cost_volume):
    """pf:239-272."""
    vl, was_np = _dev(left_cost_volume)
    vr, _ = _dev(right_cost_volume)
    return _ret(sd.wta(vl), was_np), _ret(sd.wta(vr), was_np)


def interpolation(left_disparity_map, right_disparity_map, ndisp):
    """pf:279-378."""
    dl, was_np = _dev(left_disparity_map)
    dr, _ = _dev(right_disparity_map)
    st = sd.lr_status(dl, dr, int(ndisp))
    return _ret(sd.interpolate(dl, st, directions=INTERPOLATION_DIRECTIONS, occlusion_from_left=OCCLUSION_FROM_LEFT),
                was_np)


def interpolation_right(right_disparity_map, left_disparity_map, ndisp):
    """Not in the reference: interpolation() for the RIGHT map - what it gives on the horizontally flipped pair, flipped
    back (include/mccnn.h: mccnn_lr_status_right, mccnn_interpolate_right).  Occlusions are filled from the left, and
    with OCCLUSION_FROM_LEFT (mirrored) from the right; INTERPOLATION_DIRECTIONS = 16 walks the mirrored rays.  The
    later stages are view-agnostic: subpixel_enhance, median_filter and bilateral_filter take the right view's map,
    volume and image as they are."""
    dr, was_np = _dev(right_disparity_map)
    dl, _ = _dev(left_disparity_map)
    st = sd.lr_status_right(dr, dl, int(ndisp))
    return _ret(sd.interpolate_right(dr, st, directions=INTERPOLATION_DIRECTIONS,
                                     occlusion_from_right=OCCLUSION_FROM_LEFT), was_np)


def subpixel_enhance(left_disparity_map, left_cost_volume):
    """pf:381-400."""
    dl, was_np = _dev(left_disparity_map)
    v, _ = _dev(left_cost_volume)
    return _ret(sd.subpixel(dl, v, numpy1_promotion=NUMPY1_PROMOTION), was_np)


def median_filter(left_disparity_map, filter_height, filter_width):
    """pf:403-421."""
    dl, was_np = _dev(left_disparity_map)
    return _ret(sd.median(dl, int(filter_height), int(filter_width)), was_np)


def bilateral_filter(left_image, left_disparity_map, filter_height, filter_width, mean, std_dev, blur_threshold):
    """pf:424-470."""
    img, _ = _img(left_image)
    dl, was_np = _dev(left_disparity_map)
    return _ret(sd.bilateral(img, dl, int(filter_height), int(filter_width), mean, std_dev, blur_threshold), was_np)


CONFIDENCE_MEASURES = sd.CONFIDENCE_MEASURES


def confidence_measures(left_cost_volume, right_disparity_map=None, measures=CONFIDENCE_MEASURES, view="left"):
    """Not in the reference: how far each pixel of the left winner-take-all map can be trusted (include/mccnn.h has the
    definitions; larger is more confident).  left_cost_volume: the final left volume [D,H,W] that disparity_prediction
    reads; right_disparity_map: its right map, needed by "lrc" alone.  Returns {measure: [H,W] float32 map}.
    view="right": the measures of the RIGHT map - the first argument is then the final right volume and the second the
    LEFT winner-take-all map ("lrc" looks it up at column w + d1)."""
    if view not in ("left", "right"):
        raise ValueError("view must be 'left' or 'right'")
    v, was_np = _dev(left_cost_volume)
    dr = None if right_disparity_map is None else _dev(right_disparity_map)[0]
    names = sd.confidence_names(measures)
    planes = sd.confidence(v, dr, names, view=view)
    return dict((n, _ret(planes[i].clone(), was_np)) for i, n in enumerate(names))


def semi_dense(disparity_map, rule, status=None, planes=None, measures=()):
    """Not in the reference: the semi-dense map of `disparity_map` under `rule` (a stereo_device.SemiDenseRule or its text,
    e.g. "lr,speckle:20:1"; include/mccnn.h has the definitions): kept pixels keep their bits, dropped ones hold +inf.
    status: the int32 [H,W] left-right status of the map (0 = match), needed by `lr`; planes: the confidence planes the
    rule reads - {measure: [H,W] map} as confidence_measures() returns them, or a [K,H,W] array in the order of
    `measures`."""
    rule = sd.SemiDenseRule.parse(rule)
    d, was_np = _dev(disparity_map)
    if isinstance(planes, dict):
        measures = sd.confidence_names(tuple(planes))
        planes = torch.stack([_dev(planes[n])[0] for n in measures])
    elif planes is not None:
        measures, planes = sd.confidence_names(measures), _dev(planes)[0]
    if status is None or torch.is_tensor(status):
        st = None if status is None else status.to(device=d.device, dtype=torch.int32).contiguous()
    else:
        st = torch.from_numpy(np.ascontiguousarray(status, dtype=np.int32)).to(d.device)
    return _ret(sd.semi_dense(d, rule, st, planes, measures), was_np)


def speckle_filter(disparity_map, min_size, max_diff=1.0, return_sizes=False):
    """Not in the reference: drops (+inf) every pixel whose 4-connected component - neighbours both valid and no further
    apart than max_diff - has fewer than min_size pixels.  return_sizes: -> (map, uint32 [H,W] component sizes)."""
    d, was_np = _dev(disparity_map)
    out, sizes = sd.speckle_filter(d, min_size, max_diff, want_sizes=return_sizes)
    if not return_sizes:
        return _ret(out, was_np)
    return _ret(out, was_np), (sizes.cpu().numpy().view(np.uint32) if was_np else sizes)


def depth_from_disparity(disparity_map, calib):
    """Not in the reference: the depth plane of `disparity_map` under `calib` (a calibration.Calibration or its text
    "fx,fy,cx,cy,baseline[,doffs]"; include/mccnn.h has the definitions): Z = fx * baseline / (d + doffs) in the unit of
    the baseline, +inf where the pixel has no depth."""
    d, was_np = _dev(disparity_map)
    return _ret(sd.depth(d, calib), was_np)


def reproject(disparity_map, calib, max_depth=float("inf")):
    """Not in the reference: the ordered point cloud of `disparity_map` under `calib`: float32 [n,4], one record (X, Y, Z,
    the bits of the uint32 pixel index h * W + w) per pixel with a finite Z <= max_depth, in raster order.  Reads the
    number of points back: one host synchronisation."""
    d, was_np = _dev(disparity_map)
    points, n = sd.reproject(d, calib, max_depth)
    return _ret(points[:int(n.cpu().numpy().view(np.uint32)[0])], was_np)
