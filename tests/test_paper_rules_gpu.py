"""GPU: the three opt-in rules of the paper at the edges of their kernels and through a whole pair,
bit for bit against tests/paper_rules_reference.py (which test_paper_rules_cpu.py pins to the literal loops of
test_extras_gpu.py, to post_reference.py and to the oracle).  uint32 comparison throughout; no pixel, no case left out.

kernel -> test
  cbca_both_views_kernel<13,32>   test_both_view_aggregation[short-*]: one tile less / exactly / more than one, 3 x 3 tiles
  cbca_both_views_kernel<31,16>   test_both_view_aggregation[long-*], test_unknown_plane_is_clamped_not_trusted
  mccnn_cbca_iter_both            test_both_view_refusals
  interpolate_paper_kernel        test_paper_interpolation[*] (rows around one 256-thread block, 16 status x value kinds)
  median_upto4 (all three users)  test_paper_interpolation (NaN neighbours), test_plain_interpolation_nan_neighbours
  subpixel_kernel<true>, subpixel_hwd_kernel<true>   test_numpy1_subpixel[*]
  the matcher's routes            test_whole_pair[*] (eager, stage by stage; capture; replay), test_match_cli_paper_flags"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import paper_rules_reference as pr
from conftest import GOLDEN_DIR, ROOT
from helpers import Tally, _describe, assert_bits, bits_strict

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _rc(lib, rc, code, text):
    assert rc == code, "returned %d, expected %d (%s)" % (rc, code, lib.mccnn_last_error_string())
    assert text in lib.mccnn_last_error_string(), lib.mccnn_last_error_string()


# ---- two-view aggregation ---------------------------------------------------------------------------------------------
BOTH_CASES = [("short",) + c for c in pr.BOTH_SHAPES_SHORT] + [("long",) + c for c in pr.BOTH_SHAPES_LONG]


@pytest.mark.parametrize("case", BOTH_CASES, ids=["%s-%dx%dx%d-L%d" % c for c in BOTH_CASES])
def test_both_view_aggregation(case):
    """4 image pairs x 3 volumes x 2 sides, after 1 and after 3 iterations (the ping-pong of sd.cbca_both_views), against
    both_views_iter on the arms read back from the device.  D = W + 2: the planes d >= W have no partner anywhere and
    equal the reference-order kernel's."""
    import _hipabi as hip
    import stereo_device as sd
    _, H, W, D, L = case
    R = pr.clamp_of(L)
    assert (R == 13) == (case[0] == "short")
    t = Tally("two-view aggregation %dx%dx%d L=%d" % (H, W, D, L))
    for pi, pair in enumerate(pr.IMAGE_PAIRS):
        a, b = pr.image_pair(pair, H, W, pi)
        sups = sd.cross_arms(dev(a), pr.CBCA_TAU, L), sd.cross_arms(dev(b), pr.CBCA_TAU, L)
        arms = host(sd.support_arms(sups[0])), host(sd.support_arms(sups[1]))
        if pair == "constant/constant":
            # every arm is L - 1 or the border: regions cross every tile seam, in both views and on all four sides
            for k in arms:
                for side, reach in enumerate((H, H, W, W)):
                    assert int(k[..., side].max()) == min(L, reach) - 1, (pair, side)
        for vk in pr.VOLUME_KINDS:
            vol = pr.volume(vk, D, H, W, pi)
            for side, own, other in ((hip.MCCNN_SIDE_LEFT, 0, 1), (hip.MCCNN_SIDE_RIGHT, 1, 0)):
                what = "%s %s side %d" % (pair, vk, side)
                want = pr.both_views_iter(vol, arms[own], arms[other], side, R)
                got, _ = sd.cbca_both_views(dev(vol), torch.empty((D, H, W), device="cuda"), sups[own], sups[other], 1, L,
                                            side)
                got = host(got)
                t.bits(got, want, what + ", 1 iteration")
                if vk == "special":          # a plane of -0.0: the sum starts from +0.0
                    t.check(bool((got[D // 2].view(np.uint32) == 0).all()), what + ": a mean of -0.0 is +0.0")
                if D > W:
                    ref, _ = sd.cbca(dev(vol), torch.empty((D, H, W), device="cuda"), sups[own], 1, L,
                                     hip.MCCNN_CBCA_REFERENCE_ORDER)
                    t.bits(got[W:], host(ref)[W:], what + ": planes without a partner against mccnn_cbca_iter")
                want = pr.both_views(want, arms[own], arms[other], side, R, 2)
                got, _ = sd.cbca_both_views(dev(vol), torch.empty((D, H, W), device="cuda"), sups[own], sups[other], 3, L,
                                            side)
                t.bits(host(got), want, what + ", 3 iterations")
    t.settle(floor=len(pr.IMAGE_PAIRS) * len(pr.VOLUME_KINDS) * 2 * 2)


def _unregistered_copy(support):
    """The arms of a plane at an address mccnn_cross_arms has never written (16 bytes into a fresh allocation: no
    support buffer starts there, and the plane keeps the 16-byte alignment every support pointer must have)."""
    H, W = support.shape
    room = torch.empty((H * W + 4,), dtype=torch.int32, device="cuda")
    copy = room[4:].view(H, W)
    assert copy.data_ptr() % 16 == 0 and copy.data_ptr() != room.data_ptr()
    copy.copy_(support)
    return copy


@pytest.mark.parametrize("side", [0, 1])
def test_unknown_plane_is_clamped_not_trusted(side):
    """The kernel's min(arm, R) is its memory-safety contract: a plane built with L = 32 that the registry cannot
    recognise, passed with L = 14, gives the restatement with own arms clamped to 13."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W, D = 33, 65, 7
    img = dev(pr.image_pair("constant/constant", H, W, 0)[0])
    built = sd.cross_arms(img, pr.CBCA_TAU, 32)
    arms = host(sd.support_arms(built))
    assert int(arms.max()) == 31
    copy = _unregistered_copy(built)
    vol = pr.volume("random", D, H, W, 5)
    out = torch.empty((D, H, W), device="cuda")
    rc = lib.mccnn_cbca_iter_both(hip.ptr(dev(vol)), hip.ptr(out), hip.ptr(copy), hip.ptr(copy), D, H, W, 14, side,
                                  hip.stream())
    assert rc == 0, lib.mccnn_last_error_string()
    assert_bits(host(out), pr.both_views_iter(vol, arms, arms, side, 13), "L = 32 plane at an unknown address, L = 14")
    assert not bits_strict(host(out), pr.both_views_iter(vol, arms, arms, side, 31))


def test_both_view_refusals():
    """Nothing is launched for a refused call: the output keeps its canary."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W, D = 20, 30, 3
    img = dev(pr.image_pair("synthetic", H, W, 0)[0])
    s14, s20, other_size = (sd.cross_arms(img, pr.CBCA_TAU, 14), sd.cross_arms(img, pr.CBCA_TAU, 20),
                            sd.cross_arms(img.reshape(15, 40), pr.CBCA_TAU, 14))
    vol = dev(pr.volume("random", D, H, W, 0))
    out = torch.full((D, H, W), -77.0, device="cuda")
    s = hip.stream()

    def call(src, dst, own, other, D_, L, side):
        return lib.mccnn_cbca_iter_both(hip.ptr(src), hip.ptr(dst), hip.ptr(own), hip.ptr(other), D_, H, W, L, side, s)

    _rc(lib, call(vol, vol, s14, s14, D, 14, 0), E_INVALID, b"mccnn_cbca_iter_both: in-place aggregation is not defined")
    _rc(lib, call(vol, out, s14, s14, D, 14, 2), E_INVALID, b"mccnn_cbca_iter_both: side 2")
    _rc(lib, call(vol, out, s14, s14, D, 0, 0), E_UNSUPPORTED, b"mccnn_cbca_iter_both: L=0 outside [1,32]")
    _rc(lib, call(vol, out, s14, s14, D, 33, 0), E_UNSUPPORTED, b"mccnn_cbca_iter_both: L=33 outside [1,32]")
    _rc(lib, call(vol, out, s14, s14, 65536, 14, 0), E_UNSUPPORTED, b"mccnn_cbca_iter_both: D=65536 exceeds grid.z")
    for own, other in ((s20, s14), (s14, s20)):
        _rc(lib, call(vol, out, own, other, D, 14, 1), E_INVALID,
            b"mccnn_cbca_iter_both: support plane was built with distance 20, called with L=14")
    for own, other in ((other_size, s14), (s14, other_size)):
        _rc(lib, call(vol, out, own, other, D, 14, 0), E_INVALID,
            b"mccnn_cbca_iter_both: support plane was built for a 40x15 image, volume is 30x20")
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    assert call(vol, out, s14, s14, D, 14, 0) == 0 and call(vol, out, s20, s14, D, 20, 1) == 0
    torch.cuda.synchronize()
    assert not bool((out == -77.0).any())


# ---- interpolation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(pr.INTERP_SHAPES)), ids=["%dx%d" % s for s in pr.INTERP_SHAPES])
def test_paper_interpolation(si):
    """mccnn_interpolate_ex in its four modes on 8 status kinds x 2 value kinds (test_paper_rules_cpu.py asserts that
    this set reaches every neighbour count 0 .. 16); (4, right) also through mccnn_interpolate."""
    import _hipabi as hip
    lib = hip.load()
    H, W = pr.INTERP_SHAPES[si]
    t = Tally("interpolation %dx%d" % (H, W))
    for sk, mk, dl, st in pr.interpolation_cases(si):
        ddl, dst = dev(dl), dev(st)
        for directions, occ in pr.INTERP_MODES:
            want = pr.interpolate_ex(dl, st, directions, occ)
            out = torch.empty_like(ddl)
            rc = lib.mccnn_interpolate_ex(hip.ptr(ddl), hip.ptr(dst), H, W, directions, 1 if occ else 0, hip.ptr(out),
                                          hip.stream())
            assert rc == 0, lib.mccnn_last_error_string()
            t.bits(host(out), want, "%s %s (%d, %s)" % (sk, mk, directions, occ))
            if (directions, occ) == (4, False):
                out = torch.empty_like(ddl)
                assert lib.mccnn_interpolate(hip.ptr(ddl), hip.ptr(dst), H, W, hip.ptr(out), hip.stream()) == 0
                t.bits(host(out), want, "%s %s mccnn_interpolate" % (sk, mk))
    t.settle(floor=len(pr.STATUS_KINDS) * len(pr.MAP_KINDS) * 5)


@pytest.mark.parametrize("W", [16384, 16385])
def test_plain_interpolation_nan_neighbours_wide_rows(W):
    """The reference's rule with free status maps and special values at matched pixels, at the last width of
    interpolate_row_kernel and the first of interpolate_kernel: the whole map against interpolate_ex(4, right), which the
    CPU file pins to post_reference.interpolate (that one builds a list per pixel and row: hours at this width).  The
    status maps are the two random kinds - one pixel in three is a match, so the restatement's walks stay short."""
    import stereo_device as sd
    H = 3
    t = Tally("plain interpolation, W=%d" % W)
    for ki, sk in enumerate(("random", "odd_words")):
        rng = pr.case_rng(32, W, ki)
        dl, st = pr.disparity_map("special", H, W, rng), pr.status_map(sk, H, W, rng)
        want, counts = pr.interpolate_ex(dl, st, 4, False, return_counts=True)
        assert set(np.unique(counts[counts >= 0]).tolist()) >= {2, 3, 4}
        assert int((np.isnan(want) & (st == 1) & ~np.isnan(dl)).sum()) > 100        # medians a NaN neighbour decides
        t.bits(host(sd.interpolate(dev(dl), dev(st))), want, sk)
    t.settle(floor=2)


# ---- sub-pixel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", pr.SUBPIXEL_D)
def test_numpy1_subpixel(D):
    """Both layouts (D = 2 .. 257: pitches with and without padding) x 5 kinds of cost curve; `huge` shows that the
    promotion is applied: the float32 denominator overflows there, the float64 one does not."""
    import stereo_device as sd
    t = Tally("NumPy-1 sub-pixel, D=%d" % D)
    for kind in pr.CURVE_KINDS:
        d, vol = pr.subpixel_case(D, kind)
        want = pr.subpixel_numpy1(d, vol)
        dd, dv = dev(d), dev(vol)
        got = host(sd.subpixel(dd, dv, numpy1_promotion=True))
        t.bits(got, want, "%s plane-major" % kind)
        t.bits(host(sd.subpixel_hwd(dd, sd.dhw_to_hwd(dv), D, numpy1_promotion=True)), want, "%s pixel-major" % kind)
        if kind == "huge" and D >= 12:
            plain = host(sd.subpixel(dd, dv))
            t.check(bool(((plain == d) & (got != d)).any()), "huge: the float32 chain loses pixels the promoted one keeps")
    t.settle(floor=2 * len(pr.CURVE_KINDS))


# ---- a whole pair -----------------------------------------------------------------------------------------------------
PAIR_H, PAIR_W, PAIR_D = 40, 72, 10
PAIR_HP = dict(cbca_num_iterations2=4)                  # keeps the NumPy chain short
EXTRAS = {
    "paper": dict(both_view_support=True, interpolation_directions=16, occlusion_from_left=True, numpy1_promotion=True,
                  sgm_independent_directions=True),                                 # plane-major route
    "post_only": dict(interpolation_directions=16, occlusion_from_left=True, numpy1_promotion=True),    # pixel-major
    "support_only": dict(both_view_support=True),
}


class _World(object):
    """One pair as match.py reads it from its files, the GPU's features of it, and the CPU chain per extras set."""

    def __init__(self, root, net_layers):
        import oracle as o
        import util
        from model import NET
        from test_cli_gpu import _write_pair
        self.data = os.path.join(root, "data")
        self.rel = "trainingH/pairP"
        _write_pair(os.path.join(self.data, self.rel), PAIR_H, PAIR_W, PAIR_D, seed=31)
        views = []
        for name in ("im0.png", "im1.png"):                  # match.py's decode + standardisation
            g = util.read_gray(os.path.join(self.data, self.rel, name)).astype(np.float32)
            views.append(np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2))
        self.L, self.R = views
        self.net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
        assert self.net.supports_split_features()
        fl, fr = (host(f) for f in self.net.features_pair_hwc_split(dev(self.L[:, :, 0]), dev(self.R[:, :, 0])))
        self.cv = o.compute_cost_volume(fl, fr, PAIR_D)
        self._chains = {}

    def chain(self, name):
        if name not in self._chains:
            self._chains[name] = pr.match_paper(self.L, self.R, self.cv[0], self.cv[1], PAIR_D, EXTRAS[name], PAIR_HP)
        return self._chains[name]


@pytest.fixture(scope="module")
def world(tmp_path_factory, net_layers):
    return _World(str(tmp_path_factory.mktemp("paper_pair")), net_layers)


def _first_difference(keep, cv, stages):
    """(name of the first stage whose output differs from the CPU chain's, what differs) or (None, None)."""
    from helpers import first_differing_stage
    d, notes = {}, {}
    for k, got, want in [("cv", keep["cv"], cv)] + [(k, keep[k], stages[k]) for k in pr.STAGES]:
        got = got if isinstance(got, (tuple, list)) else (got,)
        want = want if isinstance(want, (tuple, list)) else (want,)
        assert len(got) == len(want), k
        bad = [_describe(host(g), w) for g, w in zip(got, want)
               if not (bits_strict(host(g), w) if w.dtype == np.float32 else np.array_equal(host(g), w))]
        d[k], notes[k] = (1.0 if bad else 0.0), "; ".join(bad)
    first = first_differing_stage(d)
    return first, notes.get(first)


@pytest.mark.parametrize("name", list(EXTRAS))
def test_whole_pair(world, name):
    """match(keep=...) stage by stage against the CPU chain from the same cost volume; then the final map from match()
    as it is scheduled without `keep`, from the capture and from a replay of match_graph()."""
    import stereo_device as sd
    L, R = dev(world.L), dev(world.R)
    want, stages = world.chain(name)
    m = sd.StereoMatcher(world.net, hp=PAIR_HP, extras=EXTRAS[name], on_saturation="ignore")
    assert m.features == "split_f16" and m.pixel_major() == (name == "post_only")
    keep = {}
    out = host(m.match(L, R, PAIR_D, keep=keep))
    first, note = _first_difference(keep, world.cv, stages)
    assert first is None, "%s: the first stage that differs from the CPU chain is %s (%s)" % (name, first, note)
    assert_bits(out, want, name + ": match(keep)")
    assert not m.features_saturated()
    assert_bits(host(m.match(L, R, PAIR_D)), want, name + ": match()")
    assert_bits(host(m.match_graph(L, R, PAIR_D)), want, name + ": match_graph(), capture")
    assert_bits(host(m.match_graph(L, R, PAIR_D)), want, name + ": match_graph(), replay")
    base = world.chain("paper")[0] if name != "paper" else pr.match_paper(
        world.L, world.R, world.cv[0], world.cv[1], PAIR_D, None, PAIR_HP)[0]
    assert not bits_strict(base, want)                  # the sets are told apart by the map


def test_match_cli_paper_flags(world, tmp_path):
    """match.py with the four paper flags writes the bits of the `paper` set's map."""
    import util
    lst = tmp_path / "list.txt"
    lst.write_text("%s/im0.png\n" % os.path.join(world.data, world.rel))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0", "--list_file", str(lst),
           "--resume", os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"), "--data_dir", world.data, "--save_dir", str(out),
           "-t", "p", "-s", "0", "-e", "0", "--cbca_num_iterations2", str(PAIR_HP["cbca_num_iterations2"]),
           "--paper_support_regions", "--paper_interpolation", "--numpy1_promotion", "--paper_sgm"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    disp = util.readPfm(str(out / "submit_p" / world.rel / "disp0MCCNN.pfm"))
    disp = disp[0] if isinstance(disp, tuple) else disp
    disp = np.asarray(disp, np.float32).reshape(PAIR_H, PAIR_W)
    assert_bits(disp, world.chain("paper")[0], "disp0MCCNN.pfm")
