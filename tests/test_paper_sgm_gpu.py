"""GPU: the paper-faithful SGM stage - four independent directions, averaged - through every layer: the accumulating
scanline kernel (mccnn_sgm_pass_accumulate) on every route of its envelope, sgm_average_independent_hwd,
process_functional.SGM_average under SGM_INDEPENDENT_DIRECTIONS, the StereoMatcher extra sgm_independent_directions on
all its routes, and match.py --paper_sgm.  Everything is compared bit for bit (helpers.assert_bits) with
tests/paper_sgm_reference.py: oracle.semi_global_matching on copies plus NumPy's float32 sum, which
tests/test_paper_sgm_cpu.py pins against the real reference's single-direction volumes."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from helpers import assert_bits, hp_of, module_setting
import paper_sgm_reference as ps
from test_accurate_cli_gpu import RELS, _pfm, _run, _standardised
from test_accurate_cli_gpu import D as CLI_D

pytestmark = pytest.mark.gpu

GIB4 = 1 << 32
SGM_HP = (2.3, 55.9, 4, 8, 0.08, 1.5)          # P1, P2, Q1, Q2, D, V (match.py's defaults)
CHOICE = {0: "L", 1: "R"}


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


@pytest.fixture(scope="module")
def net(net_layers):
    from model import NET
    return NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)


def _sgm_hp(hp):
    return [hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]


def _images_np(H, W, seed):
    """[H,W,1] images whose steps straddle the 0.08 edge threshold, so that all three penalty classes occur."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((H, W, 1)) * 0.07).astype(np.float32),
            (rng.standard_normal((H, W, 1)) * 0.07).astype(np.float32))


def _volume_np(D, H, W, seed, inf=0.0):
    """[D,H,W] costs in [-2, 2); `inf`: share of +inf voxels (never a whole pixel: d = 0 stays finite)."""
    rng = np.random.default_rng(seed)
    v = (rng.random((D, H, W), dtype=np.float32) * 4 - 2).astype(np.float32)
    if inf:
        mask = rng.random((D, H, W)) < inf
        mask[0] = False
        v[mask] = np.inf
    return v


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_average(sd, L, R, vols, sides, D, hp=SGM_HP, flags_once=False):
    """sgm_average_independent_hwd on [D,H,W] NumPy volumes (one or two jobs) -> [D,H,W] NumPy results; checks that the
    sources are unmodified and that the roles come back swapped."""
    l, r = _dev(L[:, :, 0]), _dev(R[:, :, 0])
    H, W = l.shape
    src = [sd.dhw_to_hwd(_dev(v)) for v in vols]
    before = [s.clone() for s in src]
    spare = [torch.full_like(s, float("nan")) for s in src]          # store mode must not read what the spare holds
    flags = sd.sgm_flag_planes(l, r, D, hp[4]) if flags_once else None
    res, rest = sd.sgm_average_independent_hwd(l, r, src, spare, sides, D, *hp, sd.sgm_scratch(H, W, D, l.device),
                                               flags=flags)
    assert [t.data_ptr() for t in res] == [t.data_ptr() for t in spare]
    assert [t.data_ptr() for t in rest] == [t.data_ptr() for t in src]
    for s, b in zip(src, before):
        assert torch.equal(s.view(torch.int32), b.view(torch.int32)), "the source volume was modified"
    return [sd.hwd_to_dhw(t, D).cpu().numpy() for t in res]


def _cpu_average(L, R, vol, side, hp=SGM_HP):
    return ps.sgm_independent(vol, L, R, *hp, CHOICE[side])


# ---- golden ------------------------------------------------------------------------------------------------------------
def test_sgm_average_under_the_switch_equals_the_fixtures_average(golden_cases):
    """pf.SGM_average with SGM_INDEPENDENT_DIRECTIONS from cbca1_*: (sgm_right + sgm_left + sgm_up + sgm_bottom) / 4. of
    the real reference's volumes, both sides, all cases; the arguments - NumPy arrays or device tensors - keep their
    values, and without the switch the sequential result comes back as ever."""
    import process_functional as pf
    for name, g in golden_cases:
        hp = hp_of(g)
        want = [ps.average4([g["sgm_%s_%s" % (d, s)] for d in ps.NAMES]) for s in ("l", "r")]
        a, b = g["cbca1_l"].copy(), g["cbca1_r"].copy()
        with module_setting(pf, "SGM_INDEPENDENT_DIRECTIONS", True):
            l, r = pf.SGM_average(a, b, g["left"], g["right"], *_sgm_hp(hp))
            ta, tb = _dev(a), _dev(b)
            tl, tr = pf.SGM_average(ta, tb, _dev(g["left"]), _dev(g["right"]), *_sgm_hp(hp))
        assert_bits(l, want[0], name + " left")
        assert_bits(r, want[1], name + " right")
        assert_bits(a, g["cbca1_l"], name + " left argument modified")
        assert_bits(b, g["cbca1_r"], name + " right argument modified")
        assert_bits(tl.cpu().numpy(), want[0], name + " left (device tensors)")
        assert_bits(tr.cpu().numpy(), want[1], name + " right (device tensors)")
        assert_bits(ta.cpu().numpy(), g["cbca1_l"], name + " left device argument modified")
        assert_bits(tb.cpu().numpy(), g["cbca1_r"], name + " right device argument modified")
        l, r = pf.SGM_average(a, b, g["left"], g["right"], *_sgm_hp(hp))           # the switch is off again
        assert_bits(l, g["sgm_l"], name + " sequential left")
        assert_bits(a, g["sgm_l"], name + " sequential: argument holds the result, like the reference")


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 5, 64, 130, 150, 192, 255, 256, 257, 400, 512, 700, 768, 1000, 1024])
def test_every_route_of_the_envelope_against_the_helper(sd, D):
    """Ragged H and W, long enough that every route's steps in flight wrap several times; a two-job launch and the two
    one-job launches; about 1 % of the costs +inf."""
    H, W = 41 + D % 7, 67 + D % 5
    L, R = _images_np(H, W, seed=D)
    vl, vr = _volume_np(D, H, W, seed=D + 1, inf=0.01), _volume_np(D, H, W, seed=D + 2, inf=0.01)
    want = [_cpu_average(L, R, vl, 0), _cpu_average(L, R, vr, 1)]
    both = _gpu_average(sd, L, R, [vl, vr], [0, 1], D)
    assert_bits(both[0], want[0], "D=%d two jobs, left" % D)
    assert_bits(both[1], want[1], "D=%d two jobs, right" % D)
    swapped = _gpu_average(sd, L, R, [vr, vl], [1, 0], D, flags_once=True)
    assert_bits(swapped[0], want[1], "D=%d two jobs (right first, shared flag planes), right" % D)
    assert_bits(swapped[1], want[0], "D=%d two jobs (right first, shared flag planes), left" % D)
    for vol, side in ((vl, 0), (vr, 1)):
        one = _gpu_average(sd, L, R, [vol], [side], D, flags_once=side == 1)
        assert_bits(one[0], want[side], "D=%d one job, side %d" % (D, side))


@pytest.mark.parametrize("H,W", [(1, 40), (33, 1), (1, 1), (1, 2), (2, 1)])
@pytest.mark.parametrize("D", [5, 192, 256, 600])
def test_axes_with_nothing_to_scan_contribute_the_costs(sd, H, W, D):
    """H = 1 / W = 1: the direction along that axis has a seed line only, and L = C enters the sum."""
    L, R = _images_np(H, W, seed=3)
    vl, vr = _volume_np(D, H, W, seed=4, inf=0.02), _volume_np(D, H, W, seed=5)
    got = _gpu_average(sd, L, R, [vl, vr], [0, 1], D)
    assert_bits(got[0], _cpu_average(L, R, vl, 0), "%dx%dx%d left" % (H, W, D))
    assert_bits(got[1], _cpu_average(L, R, vr, 1), "%dx%dx%d right" % (H, W, D))
    if H == 1 and W == 1:
        with np.errstate(invalid="ignore"):
            same = ps.average4([vl, vl, vl, vl])
        assert_bits(got[0], same, "1x1: four times the costs, quartered")


def test_volumes_with_many_infinities(sd):
    """+inf is inside the contract (the cost volume's border holds it): a third of the voxels, whole disparity ranges of
    some pixels but d = 0 included."""
    D, H, W = 70, 23, 31
    L, R = _images_np(H, W, seed=8)
    vl, vr = _volume_np(D, H, W, seed=9, inf=0.33), _volume_np(D, H, W, seed=10, inf=0.33)
    vl[:, 5, 7] = np.inf
    vl[0, 5, 7] = 1.0
    got = _gpu_average(sd, L, R, [vl, vr], [0, 1], D)
    assert np.isinf(got[0]).any()
    assert_bits(got[0], _cpu_average(L, R, vl, 0), "left")
    assert_bits(got[1], _cpu_average(L, R, vr, 1), "right")


# ---- single passes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 192, 256, 300])
def test_each_mode_and_direction_alone(sd, D):
    """mccnn_sgm_pass_accumulate, one launch: acc = L, acc + L and (acc + L) / 4. for each direction and side against
    oracle.semi_global_matching on a copy plus NumPy; the source and the flag planes are shared by all launches."""
    import _hipabi as hip
    H, W = 19, 47
    L, R = _images_np(H, W, seed=20 + D)
    l, r = _dev(L[:, :, 0]), _dev(R[:, :, 0])
    planes = sd.sgm_flag_planes(l, r, D, SGM_HP[4])
    p1h, p1v, p2, q1, q2, _thr = sd._sgm_penalties(*SGM_HP)
    for side in (0, 1):
        vol = _volume_np(D, H, W, seed=30 + side, inf=0.01)
        had = _volume_np(D, H, W, seed=40 + side)
        src = sd.dhw_to_hwd(_dev(vol))
        keep = src.clone()
        for i, rr in enumerate(sd.SGM_DIRECTIONS):
            Lr = ps.single_direction(vol, L, R, rr, *SGM_HP, CHOICE[side])
            with np.errstate(invalid="ignore"):
                wants = {hip.MCCNN_SGM_ACC_STORE: Lr, hip.MCCNN_SGM_ACC_ADD: had + Lr,
                         hip.MCCNN_SGM_ACC_ADD_QUARTER: (had + Lr) / np.float32(4.)}
            for mode, want in wants.items():
                acc = sd.dhw_to_hwd(_dev(had))
                sd.sgm_pass_accumulate_hwd([src], [acc], [side], D, rr, p1h if rr[0] == 0 else p1v, p2, q1, q2, mode,
                                           planes[i])
                assert_bits(sd.hwd_to_dhw(acc, D).cpu().numpy(), want, "D=%d side %d r=%s mode %d" % (D, side, rr, mode))
        assert torch.equal(src.view(torch.int32), keep.view(torch.int32)), "the source volume was modified"


def test_the_entry_point_refuses_in_place_use_on_the_device(sd):
    import _hipabi as hip
    D, H, W = 8, 6, 12
    l = torch.zeros((H, W), device="cuda")
    v = torch.zeros((H, W, sd.hwd_pitch(D)), device="cuda")
    planes = sd.sgm_flag_planes(l, l, D, 0.08)
    with pytest.raises(hip.MccnnHipError, match="overlaps"):
        sd.sgm_pass_accumulate_hwd([v], [v], [0], D, (0, 1), 2.3, 55.9, 4.0, 8.0, hip.MCCNN_SGM_ACC_STORE, planes[0])


# ---- past 4 GiB ------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("H,W,D,cut", [(1100, 1000, 1024, 100), (2100, 2100, 256, 200)], ids=["d1024", "d256"])
def test_vertical_accumulate_passes_past_4gib_equal_their_crops(sd, H, W, D, cut):
    """As tests/test_large_volume_gpu.py: the vertical passes of a volume of 4 GiB or more rebase their descriptors - two
    of them here - every few steps; the same passes on column crops below 4 GiB (the plain kernels, pinned against the
    oracle above) must give the same bits.  Left volumes (x = w - d) on the columns [0, W - cut), right volumes on
    [cut, W): the crop sees the same flag lookups as the whole image."""
    import _hipabi as hip
    from test_large_volume_gpu import _images, _volume
    Dp = sd.hwd_pitch(D)
    assert H * W * Dp * 4 >= GIB4 and H * (W - cut) * Dp * 4 < GIB4
    src = _volume(H, W, Dp, seed=D)
    had = _volume(H, W, Dp, seed=D + 7)
    l, r = _images(H, W, seed=D + 1)
    _p1h, p1v, p2, q1, q2, _thr = sd._sgm_penalties(*SGM_HP)
    planes = dict(zip(sd.SGM_DIRECTIONS, sd.sgm_flag_planes(l, r, D, SGM_HP[4])))
    cases = [((1, 0), hip.MCCNN_SIDE_LEFT, slice(0, W - cut), hip.MCCNN_SGM_ACC_STORE),
             ((-1, 0), hip.MCCNN_SIDE_LEFT, slice(0, W - cut), hip.MCCNN_SGM_ACC_ADD),
             ((1, 0), hip.MCCNN_SIDE_RIGHT, slice(cut, W), hip.MCCNN_SGM_ACC_ADD_QUARTER),
             ((-1, 0), hip.MCCNN_SIDE_RIGHT, slice(cut, W), hip.MCCNN_SGM_ACC_STORE),
             ((-1, 0), hip.MCCNN_SIDE_RIGHT, slice(cut, W), hip.MCCNN_SGM_ACC_ADD_QUARTER)]
    for rr, side, cols, mode in cases:
        whole = had.clone()
        sd.sgm_pass_accumulate_hwd([src], [whole], [side], D, rr, p1v, p2, q1, q2, mode, planes[rr])
        got = whole[:, cols].clone(memory_format=torch.contiguous_format)
        del whole
        assert not _same_bits(got[:, :, :D], had[:, cols][:, :, :D]), "the pass changed nothing"
        lc, rc = l[:, cols].contiguous(), r[:, cols].contiguous()
        crop_src = src[:, cols].clone(memory_format=torch.contiguous_format)
        crop = had[:, cols].clone(memory_format=torch.contiguous_format)
        crop_planes = dict(zip(sd.SGM_DIRECTIONS, sd.sgm_flag_planes(lc, rc, D, SGM_HP[4])))
        sd.sgm_pass_accumulate_hwd([crop_src], [crop], [side], D, rr, p1v, p2, q1, q2, mode, crop_planes[rr])
        assert _same_bits(got[:, :, :D], crop[:, :, :D]), "D=%d r=%s side %d mode %d: whole volume differs from its crop" % (
            D, rr, side, mode)
        del got, crop, crop_src, crop_planes
        torch.cuda.empty_cache()


# ---- whole pairs -------------------------------------------------------------------------------------------------------------
PAIR = (256, 256, 64)
ON = dict(sgm_independent_directions=True)


@pytest.fixture(scope="module")
def pair():
    import synthetic
    H, W, D = PAIR
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
    return L, R, _dev(L[:, :, 0].copy()), _dev(R[:, :, 0].copy())


def _stages_behind_the_cost_volume(keep, L, R, D, hp=None, what=""):
    """keep["sgm"] against the helper on keep["cbca1"]; every other stage against the oracle fed with the GPU's previous
    stage."""
    import oracle as o
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    host = lambda t: t.cpu().numpy()
    cv = [host(t) for t in keep["cv"]]
    c1 = o.cost_volume_aggregation(L, R, cv[0], cv[1], a["cbca_intensity"], a["cbca_distance"], a["cbca_num_iterations1"])
    g1 = [host(t) for t in keep["cbca1"]]
    assert_bits(g1[0], c1[0], what + "cbca1 left")
    assert_bits(g1[1], c1[1], what + "cbca1 right")
    s = ps.SGM_average_independent(g1[0], g1[1], L, R, *_sgm_hp(a))
    gs = [host(t) for t in keep["sgm"]]
    assert_bits(gs[0], s[0], what + "sgm left")
    assert_bits(gs[1], s[1], what + "sgm right")
    c2 = o.cost_volume_aggregation(L, R, gs[0], gs[1], a["cbca_intensity"], a["cbca_distance"], a["cbca_num_iterations2"])
    g2 = [host(t) for t in keep["cbca2"]]
    assert_bits(g2[0], c2[0], what + "cbca2 left")
    assert_bits(g2[1], c2[1], what + "cbca2 right")
    dl, dr = o.disparity_prediction(g2[0], g2[1])
    gdl, gdr = host(keep["wta"][0]), host(keep["wta"][1])
    assert_bits(gdl, dl, what + "wta left")
    assert_bits(gdr, dr, what + "wta right")
    assert_bits(host(keep["interp"]), o.interpolation(gdl, gdr, D), what + "interpolation")
    assert_bits(host(keep["subpixel"]), o.subpixel_enhance(host(keep["interp"]), g2[0]), what + "subpixel")
    assert_bits(host(keep["median"]), o.median_filter(host(keep["subpixel"]), 5, 5), what + "median")
    assert_bits(host(keep["bilateral"]), o.bilateral_filter(L, host(keep["median"]), 5, 5, 0, a["blur_sigma"],
                                                            a["blur_threshold"]), what + "bilateral")


def _workspace_tensor_bytes(ws):
    total = 0
    for v in ws.values():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if torch.is_tensor(t):
                total += t.numel() * t.element_size()
    return total


def test_whole_pair_stage_by_stage_and_on_every_route(sd, net, pair):
    """256x256x64 with `keep` (the joined route): the SGM stage is the helper on the GPU's own cbca1, every later stage
    the oracle on the GPU's previous stage.  Then the same final map from the default free-running chains, from the
    chains with per-pass flag kernels, from the plane-major route and from the captured graph (twice: capture, replay)."""
    L, R, l, r = pair
    H, W, D = PAIR
    keep = {}
    joined = sd.StereoMatcher(net, extras=ON).match(l, r, D, keep=keep)
    _stages_behind_the_cost_volume(keep, L, R, D)
    want = joined.cpu().numpy()
    assert_bits(keep["bilateral"].cpu().numpy(), want, "keep's final map")
    m = sd.StereoMatcher(net, extras=ON)
    assert_bits(m.match(l, r, D).cpu().numpy(), want, "free-running chains against the joined route")
    assert_bits(m.match(l, r, D).cpu().numpy(), want, "free-running chains, workspace reused")
    for kw in (dict(sgm_flags_once=False), dict(free_chains=False), dict(two_chains=False), dict(cbca_kernel="hwd")):
        assert_bits(sd.StereoMatcher(net, extras=ON, **kw).match(l, r, D).cpu().numpy(), want, "route %r" % (kw,))
    pm = sd.StereoMatcher(net, extras=ON, layout="plane_major")
    assert not pm.pixel_major()
    keep_pm = {}
    assert_bits(pm.match(l, r, D, keep=keep_pm).cpu().numpy(), want, "plane-major route")
    assert_bits(keep_pm["sgm"][0].cpu().numpy(), keep["sgm"][0].cpu().numpy(), "plane-major sgm left")
    assert_bits(keep_pm["sgm"][1].cpu().numpy(), keep["sgm"][1].cpu().numpy(), "plane-major sgm right")
    assert_bits(pm.match(l, r, D).cpu().numpy(), want, "plane-major route, no keep")
    g = sd.StereoMatcher(net, extras=ON)
    assert_bits(g.match_graph(l, r, D).cpu().numpy(), want, "match_graph (capture)")
    assert_bits(g.match_graph(l, r, D).cpu().numpy(), want, "match_graph (replay)")
    # the workspace is what it was: the passes accumulate into the spare ping-pong buffers
    off = sd.StereoMatcher(net)
    off.match(l, r, D)
    assert _workspace_tensor_bytes(m._ws[(H, W, D)]) == _workspace_tensor_bytes(off._ws[(H, W, D)])


def test_off_means_off(sd, net, pair):
    """The extra switched off explicitly returns the bits of a matcher built without extras, the extra switched on
    returns other bits - on the default route and on the plane-major one."""
    _L, _R, l, r = pair
    D = PAIR[2]
    for kw in (dict(), dict(layout="plane_major")):
        plain = sd.StereoMatcher(net, **kw).match(l, r, D).cpu().numpy()
        off = sd.StereoMatcher(net, extras=dict(sgm_independent_directions=False), **kw).match(l, r, D).cpu().numpy()
        on = sd.StereoMatcher(net, extras=ON, **kw).match(l, r, D).cpu().numpy()
        assert_bits(off, plain, "extra off %r" % (kw,))
        assert not np.array_equal(on.view(np.uint32), plain.view(np.uint32)), "the extra changed nothing %r" % (kw,)


def test_long_arms_route(sd, net, pair):
    """cbca_distance = 20 (mccnn_cbca_iter_hwd_long_pair, no aggregation programs): the chain against the oracle, and the
    map without `keep`."""
    L, R, l, r = pair
    D = PAIR[2]
    hp = dict(cbca_distance=20)
    m = sd.StereoMatcher(net, hp=hp, extras=ON)
    assert m.route(PAIR[0], PAIR[1], D) == "hwd_long"
    keep = {}
    out = m.match(l, r, D, keep=keep)
    _stages_behind_the_cost_volume(keep, L, R, D, hp=hp, what="distance 20: ")
    assert_bits(m.match(l, r, D).cpu().numpy(), out.cpu().numpy(), "distance 20 without keep")


def test_fast_and_accurate_cost_volumes(sd, net, pair, tmp_path):
    """--fast (matrix-core cost volume) and --arch accurate (decision network): other cost volumes, and from keep["cv"]
    on the same bit-exact chain with the paper's SGM stage."""
    import _hipabi as hip
    from model import ACCURATE_NET
    L, R, l, r = pair
    D = PAIR[2]
    keep = {}
    fast = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, extras=ON)
    out = fast.match(l, r, D, keep=keep)
    _stages_behind_the_cost_volume(keep, L, R, D, what="fast: ")
    assert_bits(fast.match(l, r, D).cpu().numpy(), out.cpu().numpy(), "fast without keep")
    ckpt = str(tmp_path / "accurate.npz")
    ACCURATE_NET(None, device="cpu", seed=21).save(ckpt)
    acc = sd.StereoMatcher(ACCURATE_NET(None, batch_size=1, device="cuda").restore(ckpt), extras=ON)
    H, W = 96, 128                                     # (the decision stage is the expensive one: a smaller pair)
    keep = {}
    out = acc.match(l[:H, :W].contiguous(), r[:H, :W].contiguous(), 32, keep=keep)
    _stages_behind_the_cost_volume(keep, L[:H, :W], R[:H, :W], 32, what="accurate: ")
    assert_bits(acc.match(l[:H, :W].contiguous(), r[:H, :W].contiguous(), 32).cpu().numpy(), out.cpu().numpy(),
                "accurate without keep")


# ---- windows at the real widths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", [(750, 24, 256), (1242, 20, 192), (1500, 12, 400)])
def test_sgm_stage_on_windows_of_the_real_widths(sd, W, H, D):
    """Row windows of the benchmark shapes (Middlebury half size, KITTI, 1500 x 1000 x 400): the SGM stage against the
    helper, two jobs per launch and one."""
    L, R = _images_np(H, W, seed=W)
    vl, vr = _volume_np(D, H, W, seed=W + 1, inf=0.005), _volume_np(D, H, W, seed=W + 2, inf=0.005)
    want = [_cpu_average(L, R, vl, 0), _cpu_average(L, R, vr, 1)]
    got = _gpu_average(sd, L, R, [vl, vr], [0, 1], D, flags_once=True)
    assert_bits(got[0], want[0], "%dx%dx%d left" % (W, H, D))
    assert_bits(got[1], want[1], "%dx%dx%d right" % (W, H, D))
    assert_bits(_gpu_average(sd, L, R, [vr], [1], D)[0], want[1], "%dx%dx%d right alone" % (W, H, D))


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_match_cli_paper_sgm(tmp_path, net):
    """match.py --paper_sgm writes the map of a matcher with the extra; --pipeline and --pairs_in_flight write the same
    bytes; without the flag other bytes come out."""
    import stereo_device as sd
    fast = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
    data, plain = _run(tmp_path, "paper", ["--resume", fast, "--paper_sgm"])
    _d, piped = _run(tmp_path, "paperp", ["--resume", fast, "--paper_sgm", "--pipeline"])
    _d, two = _run(tmp_path, "paper2", ["--resume", fast, "--paper_sgm", "--pairs_in_flight", "2"])
    _d, default = _run(tmp_path, "seq", ["--resume", fast])
    m = sd.StereoMatcher(net, extras=ON)
    for rel in RELS:
        for name, other in (("--pipeline", piped), ("--pairs_in_flight 2", two)):
            assert plain[rel][0] == other[rel][0], "%s: %s wrote another disp0MCCNN.pfm" % (rel, name)
            assert plain[rel][1] == other[rel][1], "%s: %s wrote another disp0MCCNN.pgm" % (rel, name)
        assert plain[rel][0] != default[rel][0], "%s: --paper_sgm changed nothing" % rel
        L, R = (_standardised(data / rel / n) for n in ("im0.png", "im1.png"))
        want = m.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), CLI_D).cpu().numpy()
        assert_bits(_pfm(plain[rel][0], tmp_path), want, "%s: --paper_sgm" % rel)
