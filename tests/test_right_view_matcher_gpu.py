"""GPU: StereoMatcher(views="both").  Index 0 of every result is the left map of a views="left" matcher, bit for bit;
index 1 is the right-view restatement (right_view_reference.post_right: the left rules on flipped arrays, then the
oracle's sub-pixel, median and bilateral stages) applied to the winner-take-all maps, the final right volume and the
right image - the oracle's own on the golden pairs, a keep= run's on the route shapes."""
import numpy as np
import pytest
import torch

import confidence_reference as cr
import envelope_grid as grid
import right_view_reference as rv
from helpers import assert_bits
from test_default_schedule_oracle_gpu import _case, dev, env  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = cr.NAMES


def host(t):
    return t.cpu().numpy()


def release(*matchers):
    torch.cuda.synchronize()
    for m in matchers:
        m._graphs, m._ws = {}, {}
        m._side = m._right = m._library_twin = None
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["ref_24x32x8_s0.npz", "ref_40x48x16_s0.npz"])
def test_whole_pairs_against_the_oracle(env, golden_cases, name):
    import synthetic
    o, sd = env["o"], env["sd"]
    g = dict(golden_cases)[name]
    L, R = g["left"], g["right"]
    D = g["cv_l"].shape[0]
    H, W = L.shape[:2]
    case = _case(env, L, R, D)
    final, st = o.match_from_features(L, R, case.fl, case.fr, D, return_all=True)
    want = rv.post_right(R, st["wta"][0], st["wta"][1], st["cbca2"][1], D)
    for a in want.values():
        assert np.isfinite(a).all()
    assert all((want["status_right"] == v).any() for v in (0, 1, 2)), "the right view of %s lacks a state" % name
    conf_l, _ = cr.confidence(st["cbca2"][0], st["wta"][1], 15)
    conf_r, _ = rv.confidence_right(st["cbca2"][1], st["wta"][0], 15)
    m = sd.StereoMatcher(env["net"], views="both", on_saturation="raise")
    mc = sd.StereoMatcher(env["net"], views="both", confidence=ALL, on_saturation="raise")
    try:
        # eager
        got = m.match(case.l, case.r, D)
        assert tuple(got.shape) == (2, H, W) and got.dtype == torch.float32
        assert got.data_ptr() != m._ws[(H, W, D)]["both"].data_ptr()
        assert_bits(host(got[0]), final, name + ": index 0, the oracle's final map")
        assert_bits(host(got[1]), want["bilateral_right"], name + ": index 1, the right view")
        # stage by stage
        keep = {}
        kept = m.match(case.l, case.r, D, keep=keep)
        assert_bits(host(kept[0]), final, name + ": keep=, index 0")
        for stage in rv.RIGHT_STAGES:
            w = want[stage]
            gk = host(keep[stage])
            if w.dtype == np.int32:
                assert gk.dtype == np.int32 and np.array_equal(gk, w), "%s: keep[%s]" % (name, stage)
            else:
                assert_bits(gk, w, "%s: keep[%s]" % (name, stage))
        assert_bits(host(keep["cbca2_right"]), st["cbca2"][1], name + ": keep[cbca2_right]")
        assert_bits(host(keep["bilateral"]), final, name + ": keep[bilateral]")
        assert_bits(host(kept[1]), want["bilateral_right"], name + ": keep=, index 1")
        # out=
        out = torch.full((2, H, W), -7.0, device="cuda")
        assert m.match(case.l, case.r, D, out=out) is out
        assert_bits(host(out), np.stack([final, want["bilateral_right"]]), name + ": out=")
        for bad in (torch.zeros((H, W), device="cuda"), torch.zeros((2, H, W + 1), device="cuda")):
            with pytest.raises(ValueError):
                m.match(case.l, case.r, D, out=bad)
        # captured, replayed twice
        static = None
        for k in range(3):
            gm = m.match_graph(case.l, case.r, D)
            static = static or gm.data_ptr()
            assert gm.data_ptr() == static
            assert_bits(host(gm), np.stack([final, want["bilateral_right"]]), "%s: match_graph call %d" % (name, k))
        # from bytes
        l8, r8 = dev(g["left_u8"]), dev(g["right_u8"])
        sl, sr = synthetic.standardize(g["left_u8"]), synthetic.standardize(g["right_u8"])
        from_floats = host(m.match(dev(sl[:, :, 0]), dev(sr[:, :, 0]), D))
        assert_bits(host(m.match_u8(l8, r8, D)), from_floats, name + ": match_u8")
        for k in range(3):
            assert_bits(host(m.match_graph_u8(l8, r8, D)), from_floats, "%s: match_graph_u8 call %d" % (name, k))
        # confidence: [2,K,H,W]
        res, planes = mc.match(case.l, case.r, D)
        assert tuple(planes.shape) == (2, 4, H, W)
        assert_bits(host(res), np.stack([final, want["bilateral_right"]]), name + ": map beside the planes")
        assert_bits(host(planes[0]), conf_l, name + ": left planes")
        assert_bits(host(planes[1]), conf_r, name + ": right planes")
        keep = {}
        mc.match(case.l, case.r, D, keep=keep)
        assert_bits(host(keep["confidence"]), conf_l, name + ": keep[confidence]")
        assert_bits(host(keep["confidence_right"]), conf_r, name + ": keep[confidence_right]")
        cout = torch.full((2, 4, H, W), -7.0, device="cuda")
        res = mc.match(case.l, case.r, D, confidence_out=cout)
        assert res[1] is cout
        assert_bits(host(cout), np.stack([conf_l, conf_r]), name + ": confidence_out=")
        with pytest.raises(ValueError):
            mc.match(case.l, case.r, D, confidence_out=torch.zeros((4, H, W), device="cuda"))
        for k in range(2):
            gm, gp = mc.match_graph(case.l, case.r, D)
            assert_bits(host(gp), np.stack([conf_l, conf_r]), "%s: match_graph planes, call %d" % (name, k))
            assert_bits(host(gm), np.stack([final, want["bilateral_right"]]), "%s: match_graph map, call %d" % (name, k))
    finally:
        release(m, mc)


@pytest.mark.parametrize("route", [dict(), dict(layout="plane_major")], ids=["default", "plane_major"])
def test_both_views_under_per_stage_timing(env, golden_cases, route):
    """views="both" with a StageTimer: the right view does not fork - its launches go to the current stream in front of
    the left view's - and the maps and planes are the untimed call's, bit for bit."""
    sd = env["sd"]
    g = dict(golden_cases)["ref_24x32x8_s0.npz"]
    D = g["cv_l"].shape[0]
    case = _case(env, g["left"], g["right"], D)
    m = sd.StereoMatcher(env["net"], views="both", confidence=ALL, on_saturation="raise", **route)
    try:
        want, want_planes = m.match(case.l, case.r, D)
        right_stream = m._right                  # (the default route's aggregation may have made it; the fork has, too)
        timer = sd.StageTimer(True)
        got, planes = m.match(case.l, case.r, D, timer=timer)
        assert_bits(host(got), host(want), "timed: maps")
        assert_bits(host(planes), host(want_planes), "timed: planes")
        torch.cuda.synchronize()
        ms = timer.summary_ms()
        for stage in ("post", "post_right", "confidence", "confidence_right"):
            assert len(ms.get(stage, ())) == 1, "%s: %d records" % (stage, len(ms.get(stage, ())))
        assert m._right is right_stream
    finally:
        release(m)


# ---- every route ------------------------------------------------------------------------------------------------------
WINDOW = (24, 750, 256)
ROUTE_SHAPES = [WINDOW, (1, 4, 2), (1, 21, 19), (14, 20, 2), (29, 67, 65)]      # H = 1, D = 2, D = W - 2 of the grid
PAPER_EXTRAS = dict(both_view_support=True, interpolation_directions=16, occlusion_from_left=True)
# option set -> (what changes the result, the routes that must agree on it)
OPTION_SETS = {
    "default": (dict(), [dict(), dict(free_chains=False), dict(two_chains=False), dict(layout="plane_major"),
                         dict(cbca_kernel="hwd")]),
    "distance20": (dict(hp=dict(cbca_distance=20)), [dict(), dict(free_chains=False), dict(layout="plane_major")]),
    "paper_sgm": (dict(extras=dict(sgm_independent_directions=True)), [dict(), dict(free_chains=False),
                                                                       dict(layout="plane_major")]),
    "paper_extras": (dict(extras=PAPER_EXTRAS), [dict(), dict(free_chains=False)]),
    "fast": (dict(cv_mode=1), [dict(), dict(free_chains=False)]),
}
_PAIRS = {}


def _pair(shape):
    if shape not in _PAIRS:
        import synthetic
        if shape == WINDOW:
            L, R = synthetic.make_pair(shape[0], shape[1], shape[2], seed=41)[:2]
        else:
            L, R = grid.make_pair(shape)
        _PAIRS[shape] = (L, R, dev(L[:, :, 0].copy()), dev(R[:, :, 0].copy()))
    return _PAIRS[shape]


@pytest.mark.parametrize("options", sorted(OPTION_SETS))
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=[grid.name(s) for s in ROUTE_SHAPES])
def test_every_route_gives_the_same_right_map(env, shape, options):
    sd = env["sd"]
    H, W, D = shape
    base, routes = OPTION_SETS[options]
    L, R, l, r = _pair(shape)
    made = []
    try:
        def matcher(**kw):
            m = sd.StereoMatcher(env["net"], **kw)
            made.append(m)
            return m
        left_only = matcher(**base)
        want_left = host(left_only.match(l, r, D))
        # the expectation from a keep= run: the restatement on its winner-take-all maps and final right volume
        keeper = matcher(views="both", **base)
        keep = {}
        kept = host(keeper.match(l, r, D, keep=keep))
        want = rv.post_right(R, host(keep["wta"][0]), host(keep["wta"][1]), host(keep["cbca2"][1]), D, hp=keeper.hp,
                             extras=keeper.extras)
        assert_bits(host(keep["cbca2_right"]), host(keep["cbca2"][1]), "keep[cbca2_right] is the right half of keep[cbca2]")
        for stage in rv.RIGHT_STAGES[1:]:
            assert_bits(host(keep[stage]), want[stage], "%s %s keep[%s]" % (grid.name(shape), options, stage))
        assert np.array_equal(host(keep["status_right"]), want["status_right"])
        assert_bits(kept[0], want_left, "%s %s keep=: left map" % (grid.name(shape), options))
        assert_bits(kept[1], want["bilateral_right"], "%s %s keep=: right map" % (grid.name(shape), options))
        del keep
        for kw in routes:
            what = "%s %s route %r" % (grid.name(shape), options, kw)
            merged = dict(base)
            merged.update(kw)
            m = matcher(views="both", **merged)
            got = host(m.match(l, r, D))
            assert_bits(got[0], want_left, what + ": left map")
            assert_bits(got[1], want["bilateral_right"], what + ": right map")
            if options == "default" and kw == {}:
                ws = m._ws[(H, W, D)]
                assert (ws["progs"] is not None) == (m.route(H, W, D) == "prog")
                got = host(m.match_graph(l, r, D))
                assert_bits(got[1], want["bilateral_right"], what + ": right map of the captured pair")
                assert_bits(got[0], want_left, what + ": left map of the captured pair")
            release(m)
    finally:
        release(*made)


@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=[grid.name(s) for s in ROUTE_SHAPES])
def test_two_pairs_in_flight(env, shape):
    """match.py --pairs_in_flight 2: two matchers, each on its own stream with its own workspace and right stream, two
    different pairs enqueued back to back, twice; both maps of both pairs equal a lone matcher's."""
    sd = env["sd"]
    H, W, D = shape
    _, _, l, r = _pair(shape)
    l2, r2 = torch.flip(l, dims=(1,)).contiguous(), torch.flip(r, dims=(1,)).contiguous()
    solo = sd.StereoMatcher(env["net"], views="both")
    left_only = sd.StereoMatcher(env["net"])
    matchers = [sd.StereoMatcher(env["net"], views="both", on_saturation="ignore") for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    try:
        want = [host(solo.match(l, r, D)), host(solo.match(l2, r2, D))]
        assert_bits(want[0][0], host(left_only.match(l, r, D)), "%s: the lone matcher's left map" % grid.name(shape))
        assert_bits(want[1][0], host(left_only.match(l2, r2, D)), "%s: the lone matcher's left map, second pair" % grid.name(shape))
        for _ in range(2):
            torch.cuda.synchronize()
            got = []
            for m, s, (a, b) in zip(matchers, streams, ((l, r), (l2, r2))):
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    got.append(m.match(a, b, D))
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(host(got[k]), want[k], "%s: pair %d of two in flight" % (grid.name(shape), k))
    finally:
        release(solo, left_only, *matchers)


@pytest.mark.parametrize("decision", ["auto", "library"])
def test_accurate_network(env, tmp_path, decision):
    """The other network: the halves workspace and the decision stage in front of the same WTA launch.  Index 0 is the
    views="left" map, index 1 the restatement on the keep= run's winner-take-all maps and final right volume; eager,
    keep= and captured."""
    from model import ACCURATE_NET
    sd = env["sd"]
    shape = (40, 48, 16)
    H, W, D = shape
    import synthetic
    L, R = synthetic.make_pair(H, W, D, seed=100)[:2]
    l, r = dev(L[:, :, 0].copy()), dev(R[:, :, 0].copy())
    ckpt = str(tmp_path / "accurate.npz")
    ACCURATE_NET(None, device="cpu", seed=21).save(ckpt)
    acc = ACCURATE_NET(None, batch_size=1, device="cuda").restore(ckpt)
    left_only = sd.StereoMatcher(acc, decision=decision)
    m = sd.StereoMatcher(acc, decision=decision, views="both", confidence=("lrc",))
    try:
        assert m.accurate and "halves" in m.workspace(H, W, D)
        want_left = host(left_only.match(l, r, D))
        keep = {}
        kept, kplanes = m.match(l, r, D, keep=keep)
        want = rv.post_right(R, host(keep["wta"][0]), host(keep["wta"][1]), host(keep["cbca2"][1]), D, hp=m.hp, extras=m.extras)
        conf_r, _ = rv.confidence_right(host(keep["cbca2"][1]), host(keep["wta"][0]), cr.LRC)
        for stage in rv.RIGHT_STAGES[1:]:
            assert_bits(host(keep[stage]), want[stage], "accurate %s keep[%s]" % (decision, stage))
        assert np.array_equal(host(keep["status_right"]), want["status_right"])
        assert_bits(host(kplanes[1]), conf_r, "accurate %s keep=: right planes" % decision)
        for what, (got, planes) in (("match()", m.match(l, r, D)), ("match_graph()", m.match_graph(l, r, D)),
                                    ("match_graph() replay", m.match_graph(l, r, D))):
            got = host(got)
            assert_bits(got[0], want_left, "accurate %s %s: left map" % (decision, what))
            assert_bits(got[1], want["bilateral_right"], "accurate %s %s: right map" % (decision, what))
            assert_bits(host(planes[1]), conf_r, "accurate %s %s: right planes" % (decision, what))
    finally:
        release(left_only, m)


def test_views_left_is_the_matcher_without_the_argument(env):
    sd = env["sd"]
    shape = (29, 67, 65)
    H, W, D = shape
    _, _, l, r = _pair(shape)
    plain = sd.StereoMatcher(env["net"])
    left = sd.StereoMatcher(env["net"], views="left")
    both = sd.StereoMatcher(env["net"], views="both", confidence=("mmn",))
    try:
        assert plain.views == "left" and not plain.both
        a, b = plain.match(l, r, D), left.match(l, r, D)
        assert tuple(a.shape) == tuple(b.shape) == (H, W)
        assert_bits(host(a), host(b), "views='left'")
        assert_bits(host(plain.match_graph(l, r, D)), host(left.match_graph(l, r, D)), "views='left', captured")
        ws_plain, ws_left = plain.workspace(H, W, D), left.workspace(H, W, D)
        assert sorted(ws_plain) == sorted(ws_left)
        assert not any(k in ws_left for k in ("status_right", "maps_right", "both"))
        ws = both.workspace(H, W, D)
        assert sorted(set(ws) - set(ws_left)) == ["both", "confidence", "maps_right", "status_right"]
        assert tuple(ws["both"].shape) == (2, H, W) and tuple(ws["confidence"].shape) == (2, 1, H, W)
        held = sum(t.numel() * t.element_size() for k in ("both", "maps_right", "status_right", "confidence") for t in [ws[k]])
        kern = both.workspace_cbca_kernel(H, W, D)
        assert held == (sd.workspace_bytes(H, W, D, True, kern, confidence=1, views="both")
                        - sd.workspace_bytes(H, W, D, True, kern))
        with pytest.raises(ValueError):
            sd.StereoMatcher(env["net"], views="right")
    finally:
        release(plain, left, both)
