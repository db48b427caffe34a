"""GPU: StereoMatcher(confidence=...) on every route the matcher has, and process_functional.confidence_measures.
Per route: the map is bit-identical to the same matcher's without the option, and the planes are bit-identical to the
restatement (tests/confidence_reference.py) applied to the final left volume and the right winner-take-all map that a
`keep=` run of the same matcher hands out."""
import os

import numpy as np
import pytest
import torch

import confidence_reference as ref
from conftest import GOLDEN_DIR
from helpers import assert_bits

pytestmark = pytest.mark.gpu

ALL = ref.NAMES
SMALL, MID, SEAM = (40, 48, 16), (60, 96, 40), (12, 264, 257)      # (H, W, D); 257: no fused winner-take-all


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_PAIRS = {}


def pair(shape, seed=0):
    import synthetic
    key = shape + (seed,)
    if key not in _PAIRS:
        H, W, D = shape
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100 + seed)
        _PAIRS[key] = (dev(L[:, :, 0].copy()), dev(R[:, :, 0].copy()))
    return _PAIRS[key]


def host(t):
    return t.cpu().numpy()


def check_route(sd, net, shape, what, **kw):
    """One matcher configuration: returns the matcher with the option (its workspace resident) and the planes."""
    H, W, D = shape
    l, r = pair(shape)
    plain = sd.StereoMatcher(net, **kw)
    want_map = host(plain.match(l, r, D))
    m = sd.StereoMatcher(net, confidence=ALL, **kw)
    assert m.confidence == ALL
    keep = {}
    kmap, kplanes = m.match(l, r, D, keep=keep)
    assert_bits(host(kmap), want_map, what + ": map of the keep= run")
    want, d1 = ref.confidence(host(keep["cbca2"][0]), host(keep["wta"][1]), 15)
    assert np.array_equal(d1.astype(np.float32), host(keep["wta"][0])), what + ": d1 is the left winner-take-all map"
    assert_bits(host(kplanes), want, what + ": planes of the keep= run")
    assert keep["confidence"] is kplanes
    got_map, got = m.match(l, r, D)
    assert_bits(host(got_map), want_map, what + ": map")
    assert_bits(host(got), want, what + ": planes")
    assert tuple(got.shape) == (4, H, W) and got.data_ptr() != m._ws[(H, W, D)]["confidence"].data_ptr()
    return m, want_map, want


@pytest.mark.parametrize("shape", [SMALL, MID, SEAM], ids=["40x48x16", "60x96x40", "12x264x257"])
def test_default_route_eager_and_out(sd, net, shape):
    H, W, D = shape
    l, r = pair(shape)
    m, want_map, want = check_route(sd, net, shape, "free chains %s" % (shape,))
    assert (D <= sd.cbca_hwd_wta_max_d()) == (D != 257)
    out = torch.full((H, W), -7.0, device="cuda")
    cout = torch.full((4, H, W), -7.0, device="cuda")
    res = m.match(l, r, D, out=out, confidence_out=cout)
    assert res[0] is out and res[1] is cout
    assert_bits(host(out), want_map, "out=")
    assert_bits(host(cout), want, "confidence_out=")
    res = m.match(l, r, D, out=out)                        # the map into `out`, the planes as a copy
    assert res[0] is out and res[1].data_ptr() != m._ws[(H, W, D)]["confidence"].data_ptr()
    assert_bits(host(res[1]), want, "out= alone")
    with pytest.raises(ValueError):
        m.match(l, r, D, confidence_out=torch.zeros((3, H, W), device="cuda"))
    # a subset, named out of order: planes in bit order
    few = sd.StereoMatcher(net, confidence=("lrc", "mmn"))
    assert few.confidence == ("mmn", "lrc")
    fmap, fplanes = few.match(l, r, D)
    assert_bits(host(fmap), want_map, "subset: map")
    assert_bits(host(fplanes), want[[1, 3]], "subset: planes")


@pytest.mark.parametrize("kw", [dict(free_chains=False), dict(two_chains=False), dict(cbca_kernel="hwd"),
                                dict(layout="plane_major"), dict(hp=dict(cbca_distance=20)),
                                dict(extras=dict(sgm_independent_directions=True)), dict(cv_mode=1),
                                dict(cv_mode=1, cbca_order=0)],
                         ids=["joined", "one_chain", "hwd_kernel", "plane_major", "distance20", "paper_sgm", "fast_cv", "fast"])
def test_other_routes(sd, net, kw):
    m, _map, _planes = check_route(sd, net, MID, "route %r" % (kw,), **kw)
    if "layout" in kw or kw.get("cbca_order") == 0:
        assert not m.pixel_major()
    if "hp" in kw:
        assert m.route(*MID) == "hwd_long"


def test_graph_replays(sd, net, golden_cases):
    """match_graph on three different pairs, then match_graph_u8: the static map and planes of every replay equal the
    eager matcher's; a matcher without the option still returns the map alone."""
    H, W, D = MID
    m = sd.StereoMatcher(net, confidence=ALL)
    eager = sd.StereoMatcher(net, confidence=ALL)
    static = None
    for seed in (0, 1, 2):
        l, r = pair(MID, seed)
        gmap, gplanes = m.match_graph(l, r, D)
        if static is None:
            static = (gmap.data_ptr(), gplanes.data_ptr())
        assert static == (gmap.data_ptr(), gplanes.data_ptr()), "the graph entries return the static buffers"
        emap, eplanes = eager.match(l, r, D)
        assert_bits(host(gmap), host(emap), "match_graph pair %d: map" % seed)
        assert_bits(host(gplanes), host(eplanes), "match_graph pair %d: planes" % seed)
    assert not np.array_equal(host(eplanes), host(eager.match(*pair(MID, 0), D)[1]))
    g = dict(golden_cases)["ref_40x48x16_s0.npz"]
    lu, ru = dev(g["left_u8"]), dev(g["right_u8"])
    emap, eplanes = eager.match_u8(lu, ru, 16)
    for _ in range(2):
        gmap, gplanes = m.match_graph_u8(lu, ru, 16)
        assert_bits(host(gmap), host(emap), "match_graph_u8: map")
        assert_bits(host(gplanes), host(eplanes), "match_graph_u8: planes")
    plain = sd.StereoMatcher(net)
    assert torch.is_tensor(plain.match_graph_u8(lu, ru, 16)) and torch.is_tensor(plain.match_u8(lu, ru, 16))
    assert_bits(host(plain.match_graph_u8(lu, ru, 16)), host(emap), "without the option")


def test_accurate_network_and_saturation_redo(sd, tmp_path):
    """The accurate network on its library route, and the redo of a saturated pair through the library twin: the planes
    are those of the repeated pair."""
    from model import ACCURATE_NET
    ckpt = str(tmp_path / "accurate.npz")
    ACCURATE_NET(None, device="cpu", seed=21).save(ckpt)
    acc = ACCURATE_NET(None, batch_size=1, device="cuda").restore(ckpt)
    check_route(sd, acc, SMALL, "accurate, library route", decision="library")
    H, W, D = SMALL
    l, r = pair(SMALL)
    m = sd.StereoMatcher(acc, decision="kernel", confidence=ALL)
    want_map, want = sd.StereoMatcher(acc, decision="library", confidence=ALL).match(l, r, D)
    m.features_saturated = lambda reset=True: True            # every pair counts as saturated: the twin takes it
    out, cout = torch.zeros((H, W), device="cuda"), torch.zeros((4, H, W), device="cuda")
    res = m.match(l, r, D, out=out, confidence_out=cout)
    assert m._library_twin is not None and m._library_twin.confidence == ALL
    assert_bits(host(res[0]), host(want_map), "redo: map")
    assert_bits(host(res[1]), host(want), "redo: planes")
    assert_bits(host(cout), host(want), "redo: confidence_out")
    gmap, gplanes = m.match_graph(l, r, D)
    assert_bits(host(gplanes), host(want), "redo behind a replay: the static planes")
    assert_bits(host(gmap), host(want_map), "redo behind a replay: the static map")


def test_workspace_bytes(sd, net):
    H, W, D = MID
    import _hipabi as hip
    lib = hip.load()
    base = sd.workspace_bytes(H, W, D)
    # the figure from its components, as the function stated them before it knew of confidence planes: four volumes, the
    # SGM scratch and four flag planes, two support buffers, the status plane and six map planes, two program buffers
    dp = (D + 3) & ~3
    parent = (4 * H * W * dp * 4 + 5 * int(lib.mccnn_sgm_scratch_bytes(H, W, D)) + 2 * int(lib.mccnn_support_bytes(H, W))
              + 7 * H * W * 4 + 2 * int(lib.mccnn_cbca_prog_bytes(D, H, W)))
    assert base == parent
    assert sd.workspace_bytes(H, W, D, confidence=0) == base
    assert sd.workspace_bytes(H, W, D, confidence=4) == base + 4 * H * W * 4
    assert sd.workspace_bytes(H, W, D, pairs_in_flight=3, confidence=2) == 3 * (base + 2 * H * W * 4)
    plain, m = sd.StereoMatcher(net), sd.StereoMatcher(net, confidence=("cur",))
    assert plain.confidence == () and "confidence" not in plain.workspace(H, W, D)
    assert tuple(m.workspace(H, W, D)["confidence"].shape) == (1, H, W)
    with pytest.raises(ValueError):
        sd.StereoMatcher(net, confidence=("pkr",))


def test_drop_in_confidence_measures(sd, golden_cases):
    import process_functional as pf
    assert pf.CONFIDENCE_MEASURES == ALL
    for name, g in golden_cases:
        vol, right = g["cbca2_l"].copy(), g["wta_r"].copy()
        want, _ = ref.confidence(vol, right, 15)
        got = pf.confidence_measures(vol, right)
        assert sorted(got) == sorted(ALL)
        for i, n in enumerate(ALL):
            assert isinstance(got[n], np.ndarray) and got[n].dtype == np.float32
            assert_bits(got[n], want[i], "%s %s" % (name, n))
        assert_bits(vol, g["cbca2_l"], "volume argument modified")
        assert_bits(right, g["wta_r"], "map argument modified")
        few = pf.confidence_measures(vol, measures=("cur", "msm"))          # no right map: no lrc
        assert sorted(few) == ["cur", "msm"]
        assert_bits(few["cur"], want[2], name + " cur alone")
        with pytest.raises(ValueError):
            pf.confidence_measures(vol, measures=("lrc",))
        dev_got = pf.confidence_measures(dev(vol), dev(right), ("mmn",))
        assert torch.is_tensor(dev_got["mmn"])
        assert_bits(host(dev_got["mmn"]), want[1], name + " device tensors")
