"""GPU: whole pairs at the edges of check_envelope (envelope_grid.py) through StereoMatcher, bit for bit against the CPU
oracle fed the GPU's own features.

The default schedule runs the full grid (138 shapes), one test per H and one for the six extras, ONE matcher per test:
its workspace and graph are reset by every change of shape, and the first shape is matched again after the last.  Per
shape: match() first (a fault is attributable before a graph is involved), then the first match_graph() and a pure
replay (_run of test_default_schedule_oracle_gpu.py, flag planes included); all six workspace maps - both WTA maps,
interpolated, sub-pixel, median, final - against the oracle's stages after match() and after the replay, since the final
map alone is constant on the narrow shapes; the per-stage schedule (a timer switches the side stream off), whose launch
names tell whether the WTA was fused; and the same pair under keep={}, where every stage - the volumes, which are never
constant, above all - must equal the oracle's.

The matcher's other routes run the reduced grid (19 shapes), one test per route.
"""
import numpy as np
import pytest
import torch

import envelope_grid as grid
from helpers import Tally, bits_strict, stagewise
from test_default_schedule_oracle_gpu import (Case, _arm, _case, _check_flags, _check_map, _matcher, _run, dev,  # noqa: F401
                                              env)

pytestmark = pytest.mark.gpu

MAPS = ("left WTA", "right WTA", "interpolated", "sub-pixel", "median", "final")
_CASES = {}


def _stage_maps(st):
    return st["wta"][0], st["wta"][1], st["interp"], st["subpixel"], st["median"], st["bilateral"]


def _assert_finite(st, what):
    """(a NaN target would hide a difference: the comparison canonicalises NaN payloads)"""
    for stage, res in st.items():
        for a in (res if isinstance(res, tuple) else (res,)):
            assert np.isfinite(a).all(), "%s: the oracle's %s is not finite" % (what, stage)


def _oracle_case(env, shape, L, R, fl, fr, hp):
    D = shape[2]
    want, st = env["o"].match_from_features(L, R, fl, fr, D, args=hp, return_all=True)
    _assert_finite(st, grid.name(shape))
    return Case(L, R, D, hp, dev(L[:, :, 0]), dev(R[:, :, 0]), fl, fr, want), st


def _shape_case(env, shape):
    """(Case, the oracle's stages) of a grid shape on the split-operand features and the default hyper-parameters:
    computed once, shared by every test that needs it and never written to."""
    if shape not in _CASES:
        L, R = grid.make_pair(shape)
        case = _case(env, L, R, shape[2])                 # the features, once; asserts that nothing saturated
        full, st = _oracle_case(env, shape, L, R, case.fl, case.fr, None)
        assert bits_strict(full.want, case.want), grid.name(shape)
        _CASES[shape] = (case, st)
    return _CASES[shape]


class _LaunchNames(object):
    """A timer that times nothing and remembers the names of the launches it was shown."""
    enabled = False

    def __init__(self):
        self.names = []

    def start(self, name):
        self.names.append(name)

    def stop(self):
        pass

    def span_start(self, name):
        pass

    def span_stop(self, name):
        pass


def _six_maps(ws, st, what, t):
    torch.cuda.synchronize()
    got = ws["maps"].cpu().numpy()
    for i, want in enumerate(_stage_maps(st)):
        t.bits(got[i], want, "%s: workspace map %d (%s)" % (what, i, MAPS[i]))


def _stagewise_keep(env, m, case, what, t):
    """The same pair under keep={}: every entry of helpers.stagewise is exactly 0.0 (cost volume, both aggregations, SGM
    and every map), and the map handed back is the oracle's."""
    keep = {}
    got = m.match(case.l, case.r, case.D, keep=keep)
    d = stagewise(keep, case.L, case.R, case.D, env["o"], hp=m.hp, features=(case.fl, case.fr))
    assert "cost_volume" in d and "sgm" in d and "bilateral" in d
    for stage, v in d.items():
        t.check(v == 0.0, "%s, keep=: %s differs from the oracle (%g)" % (what, stage, v))
    t.bits(got.cpu().numpy(), case.want, "%s, keep=: final map" % what)
    return len(d) + 1


def _default_shape(env, m, shape):
    sd = env["sd"]
    H, W, D = shape
    what = grid.name(shape)
    case, st = _shape_case(env, shape)
    assert m.route(H, W, D) == "prog", "%s: route %s" % (what, m.route(H, W, D))
    t = Tally(what)
    ws = _arm(m, case)
    _check_map(env, m, case, m.match(case.l, case.r, D), what + ", first match()")
    _six_maps(ws, st, what + ", first match()", t)
    _check_flags(env, m, ws, case, what + ", first match()")
    ws = _run(env, m, case, what)
    _six_maps(ws, st, what + ", match_graph() replay", t)
    # the per-stage schedule: everything on one stream, and its launch names say whether the WTA was fused
    seen = _LaunchNames()
    got = m.match(case.l, case.r, D, timer=seen)
    fused = "wta" not in seen.names
    assert fused == (D <= sd.cbca_hwd_wta_max_d()), "%s: WTA fused = %s (launches: %s)" % (what, fused, seen.names)
    assert ("cbca_iter_prog_pair" in seen.names) == fused, "%s: launches %s" % (what, seen.names)
    t.bits(got.cpu().numpy(), case.want, what + ", per-stage schedule: final map")
    n = _stagewise_keep(env, m, case, what, t)
    t.settle(floor=2 * len(MAPS) + 1 + n)


def _walk(shapes, one_shape, *matchers):
    """Every shape, then the first again; a shape whose comparison fails does not hide the shapes behind it (a device
    error is no AssertionError and ends the walk).  Whatever the outcome, the matchers leave no graph, workspace or
    stream behind: the frame of a failed test outlives the test, and what it holds would stay on the device beside the
    captures of the tests that follow."""
    failures = []
    try:
        for shape in tuple(shapes) + (shapes[0],):
            try:
                one_shape(shape)
            except AssertionError as e:
                failures.append("%s: %s" % (grid.name(shape), e))
    finally:
        torch.cuda.synchronize()
        for m in matchers:
            m._graphs, m._ws = {}, {}
            m._side = m._right = m._library_twin = None
        torch.cuda.synchronize()
    assert not failures, "%d of %d shapes differ:\n%s" % (len(failures), len(shapes) + 1, "\n".join(failures))


# ---------------------------------------------------------------------------------------------------------------------
# the shipped schedule, full grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", grid.HEIGHTS)
def test_default_schedule_at_the_edges(env, H):
    shapes = grid.shapes_of_height(H)
    assert len(shapes) == 11
    m = _matcher(env, on_saturation="raise")
    _walk(shapes, lambda shape: _default_shape(env, m, shape), m)


def test_default_schedule_at_the_edges_extras(env):
    m = _matcher(env, on_saturation="raise")
    _walk(grid.EXTRAS, lambda shape: _default_shape(env, m, shape), m)


# ---------------------------------------------------------------------------------------------------------------------
# the other routes, reduced grid
# ---------------------------------------------------------------------------------------------------------------------
def _route_shape(env, m, shape, case, route, fused=None):
    """match() and the pair under keep={} against the oracle chain on the route's own features and hyper-parameters."""
    H, W, D = shape
    what = "%s, %s" % (grid.name(shape), route)
    assert m.route(H, W, D) == route, "%s: route %s" % (what, m.route(H, W, D))
    ws = m.workspace(H, W, D)
    assert (ws["progs"] is not None) == (route == "prog"), what
    t = Tally(what)
    t.bits(m.match(case.l, case.r, D).cpu().numpy(), case.want, what + ": final map of match()")
    if fused is not None:
        seen = _LaunchNames()
        t.bits(m.match(case.l, case.r, D, timer=seen).cpu().numpy(), case.want, what + ": per-stage schedule")
        assert ("wta" not in seen.names) == fused, "%s: launches %s" % (what, seen.names)
    n = _stagewise_keep(env, m, case, what, t)
    t.settle(floor=1 + n)


ROUTES = {
    "hwd": (dict(cbca_kernel="hwd"), "hwd"),
    "free_chains_off": (dict(free_chains=False), "prog"),
    "two_chains_off": (dict(two_chains=False), "prog"),
    "plane_major": (dict(layout="plane_major"), "plane_major"),
}


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_other_schedules_at_the_edges(env, name):
    """cbca_kernel="hwd": the fallback for shapes the programs do not encode, with its own fused WTA;
    free_chains / two_chains off: the joined, two-volume schedule; layout="plane_major": the plane-major
    reference-order kernels and sgm_average_from_dhw (its fused first pass up to D = 256).  Same features and
    hyper-parameters as the default schedule, so the same expected stages."""
    kw, route = ROUTES[name]
    sd = env["sd"]
    m = sd.StereoMatcher(env["net"], on_saturation="raise", **kw)
    assert m.features == "split_f16" and m.pixel_major() == (route != "plane_major")

    def one(shape):
        fused = None if route == "plane_major" else shape[2] <= sd.cbca_hwd_wta_max_d()
        _route_shape(env, m, shape, _shape_case(env, shape)[0], route, fused)
    _walk(grid.REDUCED, one, m)


def test_long_arms_at_the_edges(env):
    """cbca_distance = 28: route "hwd_long", no program buffers, no fused WTA; the oracle gets the same distance."""
    hp = dict(cbca_distance=28)
    m = env["sd"].StereoMatcher(env["net"], hp=hp, on_saturation="raise")
    assert m.pixel_major() and m.hp["cbca_distance"] == 28

    def one(shape):
        base = _shape_case(env, shape)[0]
        case, _ = _oracle_case(env, shape, base.L, base.R, base.fl, base.fr, hp)
        _route_shape(env, m, shape, case, "hwd_long", fused=False)
    _walk(grid.REDUCED, one, m)


def test_library_features_at_the_edges(env):
    """features="miopen": the library convolutions on one- and five-row images (and the rest of the reduced grid); the
    oracle chain runs on those features."""
    net = env["net"]
    m = env["sd"].StereoMatcher(net, features="miopen")
    assert m.features == "miopen" and not m.saturation_checked()

    def one(shape):
        L, R = grid.make_pair(shape)
        fl, fr = (f.cpu().numpy() for f in net.features_pair_hwc(dev(L[:, :, 0]), dev(R[:, :, 0])))
        assert fl.shape == (shape[0], shape[1], 64) and np.isfinite(fl).all() and np.isfinite(fr).all(), grid.name(shape)
        case, _ = _oracle_case(env, shape, L, R, fl, fr, None)
        _route_shape(env, m, shape, case, "prog", fused=shape[2] <= env["sd"].cbca_hwd_wta_max_d())
    _walk(grid.REDUCED, one, m)


def test_match_from_bytes_at_the_edges(env):
    """match_u8 on the uint8 scenes against match() on synthetic.standardize of the same bytes (the grid's pair): the
    two maps are identical, and they are the oracle's."""
    import synthetic
    m = _matcher(env, on_saturation="raise")
    plain = _matcher(env, on_saturation="raise")

    def one(shape):
        what = grid.name(shape)
        D = shape[2]
        l8, r8 = grid.make_scene_u8(shape)
        case = _shape_case(env, shape)[0]
        assert bits_strict(synthetic.standardize(l8), case.L) and bits_strict(synthetic.standardize(r8), case.R), what
        t = Tally(what + ", match_u8")
        got = m.match_u8(torch.from_numpy(l8).cuda(), torch.from_numpy(r8).cuda(), D).cpu().numpy()
        want = plain.match(dev(synthetic.standardize(l8)[:, :, 0]), dev(synthetic.standardize(r8)[:, :, 0]), D)
        t.bits(got, want.cpu().numpy(), what + ": match_u8 against match() on the standardised bytes")
        t.bits(got, case.want, what + ": match_u8 against the oracle")
        t.settle(floor=2)
    _walk(grid.REDUCED, one, m, plain)
