"""GPU: the memory contract of include/mccnn.h, pinned with the arena harness (tests/arena.py).

Every buffer a case hands to the library is a view into one allocation, between two 64 KiB red zones, and every case runs
twice (arena.run_twice): under fill A (-inf in the red zones, in the pad entries [..., D:] of every input volume and in
every output before the call) and under fill B (a NaN).  So
  A  a pad entry that reached a result would make the two runs differ (and -inf wins every minimum, NaN every sum),
  B  a store outside a buffer changes a red zone, a load outside a buffer that reaches a result makes the runs differ,
  C  the same cases run with every float volume, image, feature tensor and map at a 4-byte-aligned base,
  D  the matcher runs on a workspace whose volume buffers hold the fills.
Expected values never come from the code under test: the CPU oracle, and tests/paper_sgm_reference.py,
paper_rules_reference.py, fast_kernels_reference.py, vertical_reference.py for what the oracle does not have.  Everything
is compared bit for bit (helpers.assert_bits) on the entries d < D; the oracle's outputs are asserted finite first.
Because every run is compared with the same reference, the runs at odd bases equal the aligned runs bit for bit.

What was read before anything ran at an odd base (section C).  The kernels in scope touch caller volumes, images,
features and maps only through vector memory instructions of 4 to 16 bytes per lane: raw buffer loads / stores b32 .. b128
(cbca_hwd.hip, cbca_hwd_long.hip, sgm.hip, the fill kernels of cost_volume.hip, buffer_load / buffer_store_dwordx{2,3,4}
of the generated aggregation kernels), global loads / stores of one float or one float4 per lane (wta_hwd_kernel,
subpixel_hwd_kernel, the transposes, the cost-volume product kernels, sgm_flags_kernel).  None loads caller data
straight into LDS or through the scalar unit.  The support planes, the aggregation programs and the SGM flag planes ARE
read by scalar loads and packed unaligned words; they are private to the library, must be 16-byte aligned, and a pointer
that is not is refused on the host before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

import arena as A
from conftest import ROOT
from helpers import Tally, assert_bits, bits_strict, stagewise
from test_default_schedule_oracle_gpu import _case, env  # noqa: F401

pytestmark = pytest.mark.gpu

TAU = 0.02
F32 = torch.float32
AGG_SHAPES = [(5, 12, 6), (4, 70, 65), (3, 134, 130), (3, 194, 190), (3, 260, 254), (3, 262, 257)]
BIG_SHAPES = [(2, 520, 513), (2, 775, 769)]
ALL_SHAPES = AGG_SHAPES + BIG_SHAPES
SMALL_SHAPES = [(5, 12, 6), (4, 70, 65)]
ODD_SHAPES = [(5, 12, 6), (3, 262, 257)]
ODD_MODS = [(4, 4), (4, 12)]                         # (inputs, outputs): base address modulo 16
ALIGNED = (0, 0)
FILL_BITS = {"A": 0xFF800000, "B": 0x7FC00001}


def _ids(shapes):
    return ["%dx%dx%d" % s for s in shapes]


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


def pitch(D):
    return (D + 3) & ~3


def hwd_np(v, fill=0.0):
    """[D,H,W] -> pixel-major [H,W,Dp] on the host (the pads hold `fill` until poison() replaces them)."""
    D, H, W = v.shape
    out = np.full((H, W, pitch(D)), fill, np.float32)
    out[..., :D] = np.transpose(v, (1, 2, 0))
    return out


def dhw_np(a, D):
    return np.ascontiguousarray(np.transpose(np.asarray(a)[..., :D], (2, 0, 1)))


def finite(*arrays):
    for a in arrays:
        assert np.isfinite(np.asarray(a)).all(), "the reference is not finite: a NaN target would hide a difference"
    return arrays[0] if len(arrays) == 1 else arrays


def arena_bytes(shape, volumes, extra=16 << 20):
    H, W, D = shape
    return volumes * (H * W * pitch(D) * 4 + 2 * A.GUARD + 64) + extra


# ---- inputs and references: computed once per shape, shared, never written to ------------------------------------------
class Data(object):
    def __init__(self, shape):
        import oracle as o
        import synthetic
        H, W, D = shape
        self.shape, self.o = shape, o
        self.L, self.R = synthetic.make_pair(H, W, max(1, min(D, W - 2)), seed=0)[:2]
        for img in (self.L, self.R):        # regions larger than one pixel, and unit regions for the skip launches
            cnt = o.cross_arms(img, TAU, 14)[1]
            assert (cnt > 1).any() and (cnt == 1).any(), shape
        rng = np.random.default_rng(H * 1000 + W + D)
        self.vl = (rng.random((D, H, W), dtype=np.float32) * 3 - 2).astype(np.float32)
        self.vr = (rng.random((D, H, W), dtype=np.float32) * 3 - 2).astype(np.float32)
        self.rng_seed = H * 1000 + W + D
        self._cache = {}

    def memo(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def agg(self, n, dist=14):
        return self.memo(("agg", n, dist), lambda: finite(*self.o.cost_volume_aggregation(
            self.L, self.R, self.vl, self.vr, TAU, dist, n)))

    def wta(self, n, dist=14):
        return self.memo(("wta", n, dist), lambda: finite(*self.o.disparity_prediction(*self.agg(n, dist))))


_DATA = {}


def data(shape):
    if shape not in _DATA:
        _DATA[shape] = Data(shape)
    return _DATA[shape]


class Bufs(object):
    """The buffers of one case: float volumes, images, features and maps at the case's bases (inputs at mods[0], outputs
    at mods[1]); the library-private buffers - support, programs, flags - always 16-byte aligned and EXACTLY the size
    their query states, so that the byte behind them is a red zone."""

    def __init__(self, arena, sd, shape, mods=ALIGNED):
        self.a, self.sd, self.shape, (self.im, self.om) = arena, sd, shape, mods
        self.H, self.W, self.D = shape
        self.Dp = pitch(self.D)
        self.lib = __import__("_hipabi").load()

    def vol_in(self, v_dhw, name, mod=None):
        return self.a.put(hwd_np(v_dhw), self.im if mod is None else mod, name=name, pads_from=self.D)

    def vol_out(self, name, mod=None):
        return self.a.take((self.H, self.W, self.Dp), F32, self.om if mod is None else mod, name=name, pads_from=self.D,
                           output=True)

    def dhw_in(self, v, name):
        return self.a.put(v, self.im, name=name)

    def dhw_out(self, name):
        return self.a.take((self.D, self.H, self.W), F32, self.om, name=name, output=True)

    def image(self, img, name):
        return self.a.put(np.ascontiguousarray(img.reshape(self.H, self.W)), self.im, name=name)

    def map_in(self, m, name):
        return self.a.put(np.ascontiguousarray(m), self.im, name=name)

    def map_out(self, name, dtype=F32):
        return self.a.take((self.H, self.W), dtype, self.om, name=name, output=True)

    def support(self, name, mod=0):
        n = int(self.lib.mccnn_support_bytes(self.H, self.W))
        assert n % 4 == 0
        buf = self.a.take((n,), torch.uint8, mod, name=name, output=True).view(torch.int32)
        return buf[:self.H * self.W].view(self.H, self.W)

    def progs(self, tag="prog", mod=0):
        n = int(self.lib.mccnn_cbca_prog_bytes(self.D, self.H, self.W))
        assert n > 0 and n % 4 == 0
        return tuple(self.a.take((n // 4,), torch.int32, mod, name="%s_%s" % (tag, s), output=True) for s in ("l", "r"))

    def flags(self, name, mod=0):
        n = int(self.lib.mccnn_sgm_scratch_bytes(self.H, self.W, self.D))
        return self.a.take((n,), torch.uint8, mod, name=name, output=True)

    def snap(self, t):
        """The defined entries of a volume as they are now (a tensor outside the arena), its pads poisoned again."""
        torch.cuda.synchronize()
        s = t[..., :self.D].clone()
        self.a.fill_tensor(t[..., self.D:])
        return s


def run(case, shape, volumes, extra=16 << 20):
    return A.run_twice(case, arena_bytes(shape, volumes, extra), "cuda")


def check_vol(t, got, want_dhw, D, what):
    t.bits(dhw_np(got, D), want_dhw, what)


# ======================================================================================================================
# the harness itself, on the device
# ======================================================================================================================
def test_the_harness_reports_planted_violations_on_the_device(sd):
    """The planted accesses go through the arena's own base tensor and stay inside its allocation."""
    H, W, D, Dp = 3, 5, 6, 8

    def make(plant):
        def case(arena):
            rng = np.random.default_rng(0)
            v = np.zeros((H, W, Dp), np.float32)
            v[..., :D] = rng.random((H, W, D), dtype=np.float32)
            vol = arena.put(v, name="vol", pads_from=D)
            out = arena.take((H, W), F32, name="out", output=True)
            arena.poison()
            out.copy_(vol[..., :D].min(-1).values)
            e = arena.entry_of(out)
            if plant == "before":
                arena.base[e.start - 4:e.start] = 1
            elif plant == "after":
                arena.base[e.start + e.nbytes:e.start + e.nbytes + 4] = 1
            elif plant == "pad":
                out[1, 2] = vol[1, 2, D]
            elif plant == "red_zone":
                ev = arena.entry_of(vol)
                out[0, 0] = arena.base[ev.start + ev.nbytes:ev.start + ev.nbytes + 4].view(F32)[0]
            return {"out": out}
        return case
    ra, rb = A.run_twice(make(None), 4 << 20, "cuda")
    assert np.array_equal(ra["out"], rb["out"])
    for plant, words in (("before", ("out", "before", "-4 .. -1")), ("after", ("out", "after", "+60 .. +63")),
                         ("pad", ("out:", "depend on the fill")), ("red_zone", ("out:", "depend on the fill"))):
        with pytest.raises(A.Violation) as e:
            A.run_twice(make(plant), 4 << 20, "cuda")
        assert all(w in str(e.value) for w in words), str(e.value)
    a = A.Arena(4 << 20, "cuda")
    for mod in (0, 4, 8, 12):
        assert a.take((7, 3), F32, base_mod16=mod).data_ptr() % 16 == mod


# ======================================================================================================================
# A + B + C: the pixel-major aggregation kernels
# ======================================================================================================================
def _cbca_hwd_case(sd, shape, mods):
    H, W, D = shape
    d = data(shape)
    fused = D <= sd.cbca_hwd_wta_max_d()

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        sl, sr = b.support("support_l"), b.support("support_r")
        one = (b.vol_in(d.vl, "one_in"), b.vol_out("one_tmp"))
        pair = (b.vol_in(d.vl, "pair_l"), b.vol_out("pair_l_tmp"), b.vol_in(d.vr, "pair_r"), b.vol_out("pair_r_tmp"))
        wta = [(b.vol_in(d.vl, "wta%d_l" % k), b.vol_out("wta%d_l_out" % k), b.vol_in(d.vr, "wta%d_r" % k),
                b.vol_out("wta%d_r_out" % k), b.map_out("wta%d_dl" % k), b.map_out("wta%d_dr" % k))
               for k in ((1, 0) if fused else ())]
        arena.poison()
        sd.cross_arms_pair(l, r, TAU, 14, sl, sr)
        res = {"support_l": (sl, None), "support_r": (sr, None)}
        res["iter_hwd x2"], _ = sd.cbca_hwd(one[0], one[1], sl, D, 2, 14)                       # mccnn_cbca_iter_hwd
        (res["iter_hwd_pair x2 l"], _), (res["iter_hwd_pair x2 r"], _) = sd.cbca_hwd_pair(
            pair[0], pair[1], sl, pair[2], pair[3], sr, D, 2, 14)                               # mccnn_cbca_iter_hwd_pair
        for k, w in zip((1, 0), wta):                                                           # ..._pair_wta, one iteration
            (vl, _), (vr, _) = sd.cbca_hwd_pair(w[0], w[1], sl, w[2], w[3], sr, D, 1, 14, wta_out=(w[4], w[5]),
                                                store_right=bool(k))
            res["wta store_right=%d l" % k], res["wta store_right=%d dl" % k], res["wta store_right=%d dr" % k] = vl, w[4], w[5]
            torch.cuda.synchronize()
            if k:
                res["wta store_right=1 r"] = vr
            else:
                assert arena.holds_fill(w[3]), "store_right = 0 wrote the right output volume"
        return res
    ra, _ = run(case, shape, 16)
    t = Tally("cbca_hwd %s at bases %s" % (shape, mods))
    import oracle as o
    for name, img in (("support_l", d.L), ("support_r", d.R)):
        words = ra[name].view(np.uint32)
        arms, cnt = o.cross_arms(img, TAU, 14)
        t.equal(np.stack([(words >> s) & 31 for s in (0, 5, 10, 15)], -1).astype(np.uint8), arms, name + " arms")
        t.equal((words >> 20).astype(np.int32), cnt, name + " counts")
    want2, want1 = d.agg(2), d.agg(1)
    check_vol(t, ra["iter_hwd x2"], want2[0], D, "mccnn_cbca_iter_hwd")
    check_vol(t, ra["iter_hwd_pair x2 l"], want2[0], D, "mccnn_cbca_iter_hwd_pair left")
    check_vol(t, ra["iter_hwd_pair x2 r"], want2[1], D, "mccnn_cbca_iter_hwd_pair right")
    if fused:
        dl, dr = d.wta(1)
        for k in (1, 0):
            check_vol(t, ra["wta store_right=%d l" % k], want1[0], D, "pair_wta store_right=%d left volume" % k)
            t.bits(ra["wta store_right=%d dl" % k], dl, "pair_wta store_right=%d left disparities" % k)
            t.bits(ra["wta store_right=%d dr" % k], dr, "pair_wta store_right=%d right disparities" % k)
        check_vol(t, ra["wta store_right=1 r"], want1[1], D, "pair_wta store_right=1 right volume")
    t.settle(floor=7 + (7 if fused else 0))


@pytest.mark.parametrize("shape", AGG_SHAPES, ids=_ids(AGG_SHAPES))
def test_cbca_hwd_pads_and_red_zones(sd, shape):
    """mccnn_cross_arms_pair, mccnn_cbca_iter_hwd, _pair, _pair_wta (store_right 1 and 0) - A and B."""
    _cbca_hwd_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_cbca_hwd_at_odd_bases(sd, shape, mods):
    _cbca_hwd_case(sd, shape, mods)


def _cbca_long_case(sd, shape, mods, dist):
    H, W, D = shape
    d = data(shape)

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        sl, sr = b.support("support_l"), b.support("support_r")
        one = (b.vol_in(d.vr, "one_in"), b.vol_out("one_tmp"))
        pair = (b.vol_in(d.vl, "pair_l"), b.vol_out("pair_l_tmp"), b.vol_in(d.vr, "pair_r"), b.vol_out("pair_r_tmp"))
        arena.poison()
        sd.cross_arms_pair(l, r, TAU, dist, sl, sr)
        res = {}
        lib = b.lib
        import _hipabi as hip
        src, dst = one
        for _ in range(2):
            hip.check(lib.mccnn_cbca_iter_hwd_long(hip.ptr(src), hip.ptr(dst), hip.ptr(sr), D, H, W, dist, hip.stream()),
                      "mccnn_cbca_iter_hwd_long")
            src, dst = dst, src
        res["long x2"] = src
        p = list(pair)
        for _ in range(2):
            hip.check(lib.mccnn_cbca_iter_hwd_long_pair(hip.ptr(p[0]), hip.ptr(p[1]), hip.ptr(sl), hip.ptr(p[2]),
                                                        hip.ptr(p[3]), hip.ptr(sr), D, H, W, dist, hip.stream()),
                      "mccnn_cbca_iter_hwd_long_pair")
            p = [p[1], p[0], p[3], p[2]]
        res["long_pair x2 l"], res["long_pair x2 r"] = p[0], p[2]
        return res
    ra, _ = run(case, shape, 8)
    t = Tally("cbca_hwd_long %s L=%d at bases %s" % (shape, dist, mods))
    want = d.agg(2, dist)
    check_vol(t, ra["long x2"], want[1], D, "mccnn_cbca_iter_hwd_long")
    check_vol(t, ra["long_pair x2 l"], want[0], D, "mccnn_cbca_iter_hwd_long_pair left")
    check_vol(t, ra["long_pair x2 r"], want[1], D, "mccnn_cbca_iter_hwd_long_pair right")
    t.settle(floor=3)


@pytest.mark.parametrize("dist", [14, 32])
@pytest.mark.parametrize("shape", AGG_SHAPES, ids=_ids(AGG_SHAPES))
def test_cbca_hwd_long_pads_and_red_zones(sd, shape, dist):
    _cbca_long_case(sd, shape, ALIGNED, dist)


@pytest.mark.parametrize("dist", [14, 32])
@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_cbca_hwd_long_at_odd_bases(sd, shape, mods, dist):
    _cbca_long_case(sd, shape, mods, dist)


def _layout(vpl):
    from test_prog_gpu import _layout as layout
    return layout(vpl)


def _cbca_prog_case(sd, shape, mods):
    """The refresh -> skip -> wta schedule through cbca_prog_pair / cbca_prog_chain: an even count starts with a refresh
    launch (which writes its INPUT: in/out), an odd one with a full launch; both go on with skip launches; a fused count
    ends with the WTA-carrying launch.  Two-volume launches and the one-volume entry points."""
    H, W, D = shape
    d = data(shape)
    fused = D <= sd.cbca_hwd_wta_max_d()
    assert sd.skip_schedule(4, False) == ["refresh", "skip", "skip", "skip"]
    assert sd.skip_schedule(3, False) == ["full", "skip", "skip"] and sd.skip_schedule(3, True) == ["full", "skip", "wta"]

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        sl, sr = b.support("support_l"), b.support("support_r")
        progs = b.progs()

        def four(tag):
            return (b.vol_in(d.vl, tag + "_l"), b.vol_out(tag + "_l_tmp"), b.vol_in(d.vr, tag + "_r"), b.vol_out(tag + "_r_tmp"))
        p4, p3 = four("pair4"), four("pair3")
        w = [four("wta%d" % k) + (b.map_out("wta%d_dl" % k), b.map_out("wta%d_dr" % k)) for k in ((1, 0) if fused else ())]
        c4, c3 = (b.vol_in(d.vl, "chain4"), b.vol_out("chain4_tmp")), (b.vol_in(d.vr, "chain3"), b.vol_out("chain3_tmp"))
        arena.poison()
        sd.cross_arms_pair(l, r, TAU, 14, sl, sr)
        sd.cbca_prog_build_pair(sl, sr, D, 14, progs, "both")                   # mccnn_cbca_prog_build_both_pair
        res = {}
        (res["pair x4 l"], _), (res["pair x4 r"], _) = sd.cbca_prog_pair(p4[0], p4[1], sl, p4[2], p4[3], sr, progs, D, 4, 14)
        (res["pair x3 l"], _), (res["pair x3 r"], _) = sd.cbca_prog_pair(p3[0], p3[1], sl, p3[2], p3[3], sr, progs, D, 3, 14)
        for k, x in zip((1, 0), w):
            (vl, _), (vr, _) = sd.cbca_prog_pair(x[0], x[1], sl, x[2], x[3], sr, progs, D, 3, 14, wta_out=(x[4], x[5]),
                                                 store_right=bool(k))
            res["wta store_right=%d l" % k], res["wta store_right=%d dl" % k], res["wta store_right=%d dr" % k] = vl, x[4], x[5]
            if k:
                res["wta store_right=1 r"] = vr
        res["chain x4"], _ = sd.cbca_prog_chain(c4[0], c4[1], sl, progs[0], D, 4, 14)      # _refresh, _skip x3
        res["chain x3"], _ = sd.cbca_prog_chain(c3[0], c3[1], sr, progs[1], D, 3, 14)      # mccnn_cbca_iter_prog, _skip x2
        return res
    ra, _ = run(case, shape, 24)
    t = Tally("cbca_prog %s at bases %s" % (shape, mods))
    w4, w3 = d.agg(4), d.agg(3)
    check_vol(t, ra["pair x4 l"], w4[0], D, "refresh + 3 skip launches, left")
    check_vol(t, ra["pair x4 r"], w4[1], D, "refresh + 3 skip launches, right")
    check_vol(t, ra["pair x3 l"], w3[0], D, "full + 2 skip launches, left")
    check_vol(t, ra["pair x3 r"], w3[1], D, "full + 2 skip launches, right")
    check_vol(t, ra["chain x4"], w4[0], D, "one-volume refresh + 3 skip launches")
    check_vol(t, ra["chain x3"], w3[1], D, "one-volume full + 2 skip launches")
    if fused:
        dl, dr = d.wta(3)
        for k in (1, 0):
            check_vol(t, ra["wta store_right=%d l" % k], w3[0], D, "full + skip + wta, store_right=%d, left volume" % k)
            t.bits(ra["wta store_right=%d dl" % k], dl, "full + skip + wta, store_right=%d, left disparities" % k)
            t.bits(ra["wta store_right=%d dr" % k], dr, "full + skip + wta, store_right=%d, right disparities" % k)
        check_vol(t, ra["wta store_right=1 r"], w3[1], D, "full + skip + wta, store_right=1, right volume")
    t.settle(floor=6 + (7 if fused else 0))


@pytest.mark.parametrize("shape", AGG_SHAPES, ids=_ids(AGG_SHAPES))
def test_cbca_prog_pads_and_red_zones(sd, shape):
    """mccnn_cbca_iter_prog, _pair, _skip, _pair_skip, _refresh, _pair_refresh, _pair_wta on all three code versions (two,
    three and four disparities per lane by the shapes)."""
    _cbca_prog_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_cbca_prog_at_odd_bases(sd, shape, mods):
    _cbca_prog_case(sd, shape, mods)


# ======================================================================================================================
# A + B + C: SGM
# ======================================================================================================================
class SgmData(object):
    def __init__(self, shape):
        import oracle as o
        from test_paper_sgm_gpu import CHOICE, SGM_HP, _images_np, _volume_np
        H, W, D = shape
        self.o, self.hp, self.choice = o, SGM_HP, CHOICE
        self.L, self.R = _images_np(H, W, seed=D)            # steps either side of the edge threshold: all penalty classes
        self.vols = [_volume_np(D, H, W, seed=D + 1 + side) for side in (0, 1)]
        self.had = [_volume_np(D, H, W, seed=D + 11 + side) for side in (0, 1)]
        self._cache = {}

    def p1(self, r):
        return self.hp[0] if r[0] == 0 else self.hp[0] / self.hp[5]

    def sequence(self, side, directions):
        """The volume after each of `directions`, composed in place (pf:544)."""
        key = ("seq", side, tuple(directions))
        if key not in self._cache:
            v, outs = self.vols[side].copy(), []
            for r in directions:
                self.o.semi_global_matching(self.L, self.R, v, r, self.p1(r), *self.hp[1:5], self.choice[side])
                outs.append(finite(v.copy()))
            self._cache[key] = outs
        return self._cache[key]

    def single(self, side, r):
        import paper_sgm_reference as ps
        key = ("single", side, r)
        if key not in self._cache:
            self._cache[key] = finite(ps.single_direction(self.vols[side], self.L, self.R, r, *self.hp, self.choice[side]))
        return self._cache[key]


_SGM = {}


def sgm_data(shape):
    if shape not in _SGM:
        _SGM[shape] = SgmData(shape)
    return _SGM[shape]


def _sgm_pass_case(sd, shape, mods):
    H, W, D = shape
    d = sgm_data(shape)
    dirs = sd.SGM_DIRECTIONS
    p1h, p1v, p2, q1, q2, thr = sd._sgm_penalties(*d.hp)
    variants = [(flagged, jobs) for flagged in (False, True) for jobs in (2, 1)]

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        scratch = b.flags("scratch")
        planes = [b.flags("flags_%d" % i) for i in range(4)]
        vols = {v: [b.vol_in(d.vols[side], "vol_%s_%d_%d" % (v[0], v[1], side)) for side in (0, 1)] for v in variants}
        arena.poison()
        for i, rr in enumerate(dirs):
            sd.sgm_flags_hwd(l, r, D, rr, thr, planes[i])                                   # mccnn_sgm_flags
        res = {}
        for i, rr in enumerate(dirs):
            p1 = p1h if rr[0] == 0 else p1v
            for v in variants:
                flagged, jobs = v
                for group in ([[0, 1]] if jobs == 2 else [[1], [0]]):
                    hwd = [vols[v][s] for s in group]
                    if flagged:
                        sd.sgm_pass_flagged_hwd(hwd, group, D, rr, p1, p2, q1, q2, planes[i])       # mccnn_sgm_pass_flagged
                    else:
                        sd.sgm_pass_hwd(l, r, hwd, group, D, rr, p1, p2, q1, q2, thr, scratch)      # mccnn_sgm_pass
                for side in (0, 1):      # in/out: the pass wrote its input; its pads are poisoned again for the next one
                    res["%s %d job(s) r=%s side %d" % ("flagged" if flagged else "own flags", jobs, rr, side)] = b.snap(vols[v][side])
        return res
    ra, _ = run(case, shape, 10, extra=(64 << 20) if shape in BIG_SHAPES else (16 << 20))
    t = Tally("sgm passes %s at bases %s" % (shape, mods))
    for side in (0, 1):
        want = d.sequence(side, dirs)
        for i, rr in enumerate(dirs):
            for flagged, jobs in variants:
                name = "%s %d job(s) r=%s side %d" % ("flagged" if flagged else "own flags", jobs, rr, side)
                check_vol(t, ra[name], want[i], D, name)
    t.settle(floor=32)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids(ALL_SHAPES))
def test_sgm_passes_pads_and_red_zones(sd, shape):
    """mccnn_sgm_flags, mccnn_sgm_pass and mccnn_sgm_pass_flagged: four directions, both sides, one and two jobs, in place
    (the volume is in/out; its pads are poisoned again in front of every pass)."""
    _sgm_pass_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_sgm_passes_at_odd_bases(sd, shape, mods):
    _sgm_pass_case(sd, shape, mods)


def _sgm_accumulate_case(sd, shape, mods):
    import _hipabi as hip
    H, W, D = shape
    d = sgm_data(shape)
    dirs = sd.SGM_DIRECTIONS
    p1h, p1v, p2, q1, q2, thr = sd._sgm_penalties(*d.hp)
    modes = (("store", hip.MCCNN_SGM_ACC_STORE), ("add", hip.MCCNN_SGM_ACC_ADD), ("add_quarter", hip.MCCNN_SGM_ACC_ADD_QUARTER))

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        planes = [b.flags("flags_%d" % i) for i in range(4)]
        src = [b.vol_in(d.vols[side], "src_%d" % side) for side in (0, 1)]
        acc = [b.vol_in(d.had[side], "acc_%d" % side, mod=b.om) for side in (0, 1)]         # in/out, pad-bearing
        had = [a.clone() for a in acc]
        arena.poison()
        for i, rr in enumerate(dirs):
            sd.sgm_flags_hwd(l, r, D, rr, thr, planes[i])
        res = {}

        def launch(group, rr, i, name, mode, tag):
            for s in group:
                acc[s].copy_(had[s])
                arena.fill_tensor(acc[s][..., D:])
            sd.sgm_pass_accumulate_hwd([src[s] for s in group], [acc[s] for s in group], group, D, rr,
                                       p1h if rr[0] == 0 else p1v, p2, q1, q2, mode, planes[i])
            for s in group:
                res["%s r=%s %s side %d" % (tag, rr, name, s)] = b.snap(acc[s])
        for i, rr in enumerate(dirs):
            for name, mode in modes:
                launch([0, 1], rr, i, name, mode, "two jobs")
        for name, mode in modes:
            launch([1], dirs[2], 2, name, mode, "one job")
            launch([0], dirs[1], 1, name, mode, "one job")
        res["src_0"], res["src_1"] = src
        return res
    ra, _ = run(case, shape, 6, extra=(64 << 20) if shape in BIG_SHAPES else (16 << 20))
    t = Tally("sgm accumulate %s at bases %s" % (shape, mods))

    def wants(side, rr):
        Lr, had = d.single(side, rr), d.had[side]
        return {"store": Lr, "add": had + Lr, "add_quarter": (had + Lr) / np.float32(4.)}
    for i, rr in enumerate(dirs):
        for side in (0, 1):
            for name, want in wants(side, rr).items():
                check_vol(t, ra["two jobs r=%s %s side %d" % (rr, name, side)], finite(want), D, "%s %s side %d" % (rr, name, side))
    for side, rr in ((1, dirs[2]), (0, dirs[1])):
        for name, want in wants(side, rr).items():
            check_vol(t, ra["one job r=%s %s side %d" % (rr, name, side)], want, D, "one job %s %s side %d" % (rr, name, side))
    for side in (0, 1):
        check_vol(t, ra["src_%d" % side], d.vols[side], D, "the source volume was written")
    t.settle(floor=24 + 6 + 2)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids(ALL_SHAPES))
def test_sgm_accumulate_pads_and_red_zones(sd, shape):
    """mccnn_sgm_pass_accumulate in its three modes; the source and the accumulator are pad-bearing."""
    _sgm_accumulate_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_sgm_accumulate_at_odd_bases(sd, shape, mods):
    _sgm_accumulate_case(sd, shape, mods)


def _sgm_first_pass_case(sd, shape, mods):
    import _hipabi as hip
    H, W, D = shape
    d = sgm_data(shape)
    p1h, _p1v, p2, q1, q2, thr = sd._sgm_penalties(*d.hp)

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        scratch = b.flags("scratch")
        src = [b.dhw_in(d.vols[side], "dhw_%d" % side) for side in (0, 1)]
        two = [b.vol_out("two_%d" % side) for side in (0, 1)]
        one = [b.vol_out("one_%d" % side) for side in (0, 1)]
        arena.poison()
        lib = b.lib
        for group, dst in (([0, 1], two), ([1], one), ([0], one)):
            n, side_arr, s_arr, d_arr = sd._sgm_arrays(group, [src[s] for s in group], [dst[s] for s in group])
            hip.check(lib.mccnn_sgm_first_pass(hip.ptr(l), hip.ptr(r), s_arr, d_arr, side_arr, n, D, H, W, p1h, p2, q1, q2, thr,
                                               hip.ptr(scratch), scratch.numel(), hip.stream()), "mccnn_sgm_first_pass")
        return {"two jobs side 0": two[0], "two jobs side 1": two[1], "one job side 0": one[0], "one job side 1": one[1],
                "dhw_0": src[0], "dhw_1": src[1]}
    ra, _ = run(case, shape, 8)
    t = Tally("sgm first pass %s at bases %s" % (shape, mods))
    for side in (0, 1):
        want = d.sequence(side, sd.SGM_DIRECTIONS[:1])[0]
        check_vol(t, ra["two jobs side %d" % side], want, D, "two jobs, side %d" % side)
        check_vol(t, ra["one job side %d" % side], want, D, "one job, side %d" % side)
        t.bits(ra["dhw_%d" % side], d.vols[side], "the plane-major source was written")
    t.settle(floor=6)


FIRST_PASS_SHAPES = [x for x in AGG_SHAPES if x[2] <= 256]


@pytest.mark.parametrize("shape", FIRST_PASS_SHAPES, ids=_ids(FIRST_PASS_SHAPES))
def test_sgm_first_pass_pads_and_red_zones(sd, shape):
    """mccnn_sgm_first_pass (D <= 256): the plane-major source has no pads, the output pads start poisoned."""
    assert shape[2] <= sd.SGM_FIRST_PASS_MAX_D
    _sgm_first_pass_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
def test_sgm_first_pass_at_odd_bases(sd, mods):
    """(5, 12, 6); (3, 262, 257) is beyond the entry point's 256 disparities, (3, 260, 254) stands in for it."""
    _sgm_first_pass_case(sd, (5, 12, 6), mods)
    _sgm_first_pass_case(sd, (3, 260, 254), mods)


# ======================================================================================================================
# A + B + C: WTA, sub-pixel, layout changes, cost volume
# ======================================================================================================================
class MapData(object):
    def __init__(self, shape):
        import oracle as o
        import paper_rules_reference as ppr
        H, W, D = shape
        rng = np.random.default_rng(7 * H + W + D)
        v = (rng.random((D, H, W), dtype=np.float32) * 3 - 2).astype(np.float32)
        v[D - 1, 0, 1] = -100.0                              # the winner is D - 1: d + 1 would be the first pad
        v[D - 1, H - 1, W - 1] = -100.0
        v[[1, D // 2], 1, 2] = -50.0                         # a tie: the lower index wins
        if D > 512:
            v[[5, 300, D - 1], 1, 3] = -60.0                 # across the 256-disparity groups, the last lane included
        if D > 300:
            v[[260, 270], 0, 4] = -60.0
        self.vol = v
        self.wta = finite(o.disparity_prediction(v, v)[0])
        assert self.wta[0, 1] == D - 1 and self.wta[1, 2] == 1
        m = self.wta.copy()
        half = rng.random((H, W)) < 0.5
        half[0, 1] = half[H - 1, W - 1] = False              # these stay exactly D - 1
        m[half & (m < D - 1)] += np.float32(0.5)
        m[0, 0] = np.float32(D - 1.5)                        # reads D - 1 as its d + 1 neighbour
        self.map = m
        self.sub = finite(o.subpixel_enhance(m, v))
        self.sub1 = finite(ppr.subpixel_numpy1(m, v))
        assert self.sub[0, 1] == D - 1 and not bits_strict(self.sub, m)


_MAPS = {}


def map_data(shape):
    if shape not in _MAPS:
        _MAPS[shape] = MapData(shape)
    return _MAPS[shape]


def _wta_subpixel_case(sd, shape, mods):
    H, W, D = shape
    d = map_data(shape)

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        vol, m = b.vol_in(d.vol, "vol"), b.map_in(d.map, "map")
        outs = [b.map_out(n) for n in ("wta", "subpixel", "subpixel_numpy1")]
        dhw = b.dhw_out("dhw")
        arena.poison()
        sd.wta_hwd(vol, D, out=outs[0])
        sd.subpixel_hwd(m, vol, D, out=outs[1])
        sd.subpixel_hwd(m, vol, D, out=outs[2], numpy1_promotion=True)
        sd.hwd_to_dhw(vol, D, dhw)
        return {"wta": outs[0], "subpixel": outs[1], "subpixel_numpy1": outs[2], "dhw": dhw, "vol": vol, "map": m}
    ra, _ = run(case, shape, 3)
    t = Tally("wta / subpixel / hwd_to_dhw %s at bases %s" % (shape, mods))
    t.bits(ra["wta"], d.wta, "mccnn_wta_hwd")
    t.bits(ra["subpixel"], d.sub, "mccnn_subpixel_hwd")
    t.bits(ra["subpixel_numpy1"], d.sub1, "mccnn_subpixel_hwd, numpy1 promotion")
    t.bits(ra["dhw"], d.vol, "mccnn_hwd_to_dhw")
    check_vol(t, ra["vol"], d.vol, D, "the input volume was written")
    t.bits(ra["map"], d.map, "the input map was written")
    t.settle(floor=6)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids(ALL_SHAPES))
def test_wta_subpixel_and_layout_change_pads_and_red_zones(sd, shape):
    """mccnn_wta_hwd, mccnn_subpixel_hwd (both promotions; winners at D - 1), mccnn_hwd_to_dhw."""
    _wta_subpixel_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_wta_subpixel_and_layout_change_at_odd_bases(sd, shape, mods):
    _wta_subpixel_case(sd, shape, mods)


class CvData(object):
    def __init__(self, shape):
        import oracle as o
        import vertical_reference as vr
        H, W, D = shape
        rng = np.random.default_rng(3 * H + W + D)
        f = rng.standard_normal((2, H, W, 64)).astype(np.float32)
        f /= np.sqrt((f * f).sum(-1, keepdims=True))
        self.fl, self.fr = np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])
        self.cv = finite(*o.compute_cost_volume(self.fl, self.fr, D))
        self.cv2 = finite(*vr.compute_cost_volume_vertical(self.fl, self.fr, D, 2))
        # what the fill launch is given: the scores w >= d (left) / w + d < W (right), the border entries garbage
        dd, ww = np.arange(D)[:, None, None], np.arange(W)[None, None, :]
        self.scored = [np.where(np.broadcast_to(keep, c.shape), c, np.float32(12345.0)).astype(np.float32)
                       for c, keep in ((self.cv[0], ww >= dd), (self.cv[1], ww + dd < W))]


_CV = {}


def cv_data(shape):
    if shape not in _CV:
        _CV[shape] = CvData(shape)
    return _CV[shape]


def _cost_volume_case(sd, shape, mods):
    H, W, D = shape
    d = cv_data(shape)

    def case(arena):
        b = Bufs(arena, sd, shape, mods)
        fl, fr = arena.put(d.fl, b.im, name="features_l"), arena.put(d.fr, b.im, name="features_r")
        exact = (b.vol_out("exact_l"), b.vol_out("exact_r"))
        vert = (b.vol_out("vertical_l"), b.vol_out("vertical_r"))
        fill = (b.vol_in(d.scored[0], "fill_l", mod=b.om), b.vol_in(d.scored[1], "fill_r", mod=b.om))      # in/out
        arena.poison()
        sd.cost_volume_hwd(fl, fr, D, out=exact)                                    # MCCNN_CV_EXACT
        sd.cost_volume_vertical_hwd(fl, fr, D, 2, out=vert)
        sd.cost_volume_fill(fill[0], fill[1], D, True)
        return {"exact_l": exact[0], "exact_r": exact[1], "vertical_l": vert[0], "vertical_r": vert[1],
                "fill_l": fill[0], "fill_r": fill[1], "features_l": fl, "features_r": fr}
    ra, rb = run(case, shape, 8)
    t = Tally("cost volume %s at bases %s" % (shape, mods))
    for i, side in enumerate("lr"):
        check_vol(t, ra["exact_" + side], d.cv[i], D, "mccnn_cost_volume_hwd " + side)
        check_vol(t, ra["vertical_" + side], d.cv2[i], D, "mccnn_cost_volume_vertical_hwd " + side)
        check_vol(t, ra["fill_" + side], d.cv[i], D, "mccnn_cost_volume_fill(pixel_major=1) " + side)
        t.bits(ra["features_" + side], (d.fl, d.fr)[i], "the features were written")
        for name in ("exact_", "vertical_", "fill_"):            # the header's promise: the pads are not written
            for got, fill in ((ra, "A"), (rb, "B")):
                pads = got[name + side][..., D:].view(np.uint32)
                t.check(bool((pads == FILL_BITS[fill]).all()), "%s%s: %d pad entries lost fill %s" % (
                    name, side, int((pads != FILL_BITS[fill]).sum()), fill))
    t.settle(floor=2 * (4 + 6))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids(ALL_SHAPES))
def test_cost_volume_pads_and_red_zones(sd, shape):
    """mccnn_cost_volume_hwd (MCCNN_CV_EXACT), mccnn_cost_volume_vertical_hwd (range 2), mccnn_cost_volume_fill
    (pixel_major = 1): equal to the references, and the pads KEEP the fill."""
    _cost_volume_case(sd, shape, ALIGNED)


@pytest.mark.parametrize("mods", ODD_MODS, ids=["in4_out4", "in4_out12"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_ids(ODD_SHAPES))
def test_cost_volume_at_odd_bases(sd, shape, mods):
    _cost_volume_case(sd, shape, mods)


@pytest.mark.parametrize("which", ["dhw_aligned_hwd_odd", "dhw_odd_hwd_aligned", "both_aligned"])
def test_layout_changes_reach_the_fallback_kernels_at_n_multiple_of_4(sd, which):
    """H * W = 60, D = 6: the 16-byte transposes serve N % 4 == 0 only between two 16-byte-aligned bases; with one side at
    a 4-byte-aligned base the element-wise kernels run."""
    shape = (5, 12, 6)
    H, W, D = shape
    d = data(shape)
    dm, hm = {"dhw_aligned_hwd_odd": (0, 4), "dhw_odd_hwd_aligned": (12, 0), "both_aligned": (0, 0)}[which]

    def case(arena):
        b = Bufs(arena, sd, shape)
        dhw_in = arena.put(d.vl, dm, name="dhw_in")
        hwd_out = arena.take((H, W, pitch(D)), F32, hm, name="hwd_out", pads_from=D, output=True)
        hwd_in = arena.put(hwd_np(d.vr), hm, name="hwd_in", pads_from=D)
        dhw_out = arena.take((D, H, W), F32, dm, name="dhw_out", output=True)
        arena.poison()
        sd.dhw_to_hwd(dhw_in, hwd_out)
        sd.hwd_to_dhw(hwd_in, D, dhw_out)
        return {"hwd_out": hwd_out, "dhw_out": dhw_out}
    ra, _ = run(case, shape, 4)
    assert_bits(dhw_np(ra["hwd_out"], D), d.vl, "mccnn_dhw_to_hwd, " + which)
    assert_bits(ra["dhw_out"], d.vr, "mccnn_hwd_to_dhw, " + which)


# ======================================================================================================================
# B: entry points without pads (red zones, and nothing depends on the fill)
# ======================================================================================================================
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=_ids(SMALL_SHAPES))
def test_arms_programs_and_flags_red_zones(sd, shape):
    """mccnn_cross_arms, _pair; mccnn_cbca_prog_build_pair, _skip_pair, _both_pair; mccnn_sgm_flags: the support, program
    and flag buffers are exactly as long as their queries say and a red zone follows.  The arms against the oracle, the
    programs against the plain-Python statement (tests/asmtools/cbca_prog_ref.py), the flags through a pass."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "asmtools"))
    import cbca_prog_ref as ref
    import oracle as o
    H, W, D = shape
    d, s = data(shape), sgm_data(shape)
    lay = _layout(2)
    assert pitch(D) <= 128
    p1h, p1v, p2, q1, q2, thr = sd._sgm_penalties(*s.hp)
    # the programs the builder must write, from the ORACLE's arms; a patch's program ends with its END op and the words
    # behind it, up to the patch's stride, belong to nobody: `written` marks the defined ones
    progs_want, written = {}, {}
    for side, img in (("l", d.L), ("r", d.R)):
        arms, cnt = o.cross_arms(img, TAU, 14)
        a = arms.astype(np.uint32)
        sup0 = a[..., 0] | (a[..., 1] << 5) | (a[..., 2] << 10) | (a[..., 3] << 15) | (cnt.astype(np.uint32) << 20)
        sets, masks = [], []
        for skip in (False, True):
            want, meta = ref.build_all(sup0, H, W, lay, skip_unit=skip)
            mask = np.zeros(want.shape, bool)
            for rg in range(want.shape[0]):
                if rg * lay["K"] >= H:
                    continue
                for cg in range(want.shape[1]):
                    mask[rg, cg, :len(ref.build_program(sup0, H, W, rg * lay["K"], cg * lay["G"], lay, skip))] = True
            sets.append(want)
            masks.append(mask)
        progs_want[side], written[side] = np.stack(sets).reshape(-1), np.stack(masks).reshape(-1)
        assert written[side].any() and not written[side].all()

    def case(arena):
        b = Bufs(arena, sd, shape)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        il, ir = b.image(s.L, "sgm_left"), b.image(s.R, "sgm_right")
        one, one32 = b.support("support_single"), b.support("support_single_L32")
        sl, sr = b.support("support_l"), b.support("support_r")
        two, both = b.progs("prog_two"), b.progs("prog_both")
        planes = b.flags("flags")
        vol = b.vol_in(s.vols[0], "vol")
        arena.poison()
        sd.cross_arms(l, TAU, 14, out=one)
        sd.cross_arms(r, TAU, 32, out=one32)
        sd.cross_arms_pair(l, r, TAU, 14, sl, sr)
        sd.cbca_prog_build_pair(sl, sr, D, 14, two, "both_two_launches")
        sd.cbca_prog_build_pair(sl, sr, D, 14, both, "both")
        sd.sgm_flags_hwd(il, ir, D, (1, 0), thr, planes)
        sd.sgm_pass_flagged_hwd([vol], [0], D, (1, 0), p1v, p2, q1, q2, planes)
        torch.cuda.synchronize()
        return {"single": (one, None), "single_L32": (one32, None), "support_l": (sl, None), "support_r": (sr, None),
                "two_l": (two[0], written["l"]), "two_r": (two[1], written["r"]), "both_l": (both[0], written["l"]),
                "both_r": (both[1], written["r"]), "pass": vol}
    ra, _ = run(case, shape, 4)
    t = Tally("arms, programs, flags %s" % (shape,))
    for name, img, dist in (("single", d.L, 14), ("single_L32", d.R, 32), ("support_l", d.L, 14), ("support_r", d.R, 14)):
        words = ra[name].view(np.uint32)
        arms, cnt = o.cross_arms(img, TAU, dist)
        t.equal(np.stack([(words >> k) & 31 for k in (0, 5, 10, 15)], -1).astype(np.uint8), arms, name + " arms")
        t.equal((words >> 20).astype(np.int32), cnt, name + " counts")
    for side in "lr":
        for kind in ("two_", "both_"):
            got = ra[kind + side].view(np.uint32)
            assert got.shape == progs_want[side].shape
            t.equal(got[written[side]], progs_want[side][written[side]], kind + side + ": full and skip programs")
    check_vol(t, ra["pass"], s.sequence(0, [(1, 0)])[0], D, "mccnn_sgm_flags read by a pass")
    t.settle(floor=8 + 4 + 1)


@pytest.mark.parametrize("dist", [14, 32])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=_ids(SMALL_SHAPES))
def test_plane_major_aggregation_red_zones(sd, shape, dist):
    """mccnn_cbca_iter in both orders, mccnn_cbca_iter_both, mccnn_dhw_to_hwd.  The reference order against the oracle and
    the two-view regions against tests/paper_rules_reference.py, two iterations, bit for bit; the separable order is no
    bit-exact kernel: one iteration inside the bound include/mccnn.h states for it (fast_kernels_reference)."""
    import _hipabi as hip
    import fast_kernels_reference as fk
    import oracle as o
    import paper_rules_reference as ppr
    H, W, D = shape
    d = data(shape)

    def case(arena):
        b = Bufs(arena, sd, shape)
        l, r = b.image(d.L, "left"), b.image(d.R, "right")
        sl, sr = b.support("support_l"), b.support("support_r")
        ref_io = (b.dhw_in(d.vl, "ref_in"), b.dhw_out("ref_tmp"))
        sep_io = (b.dhw_in(d.vl, "sep_in"), b.dhw_out("sep_out"))
        both_l = (b.dhw_in(d.vl, "both_l_in"), b.dhw_out("both_l_tmp"))
        both_r = (b.dhw_in(d.vr, "both_r_in"), b.dhw_out("both_r_tmp"))
        t_in, t_out = b.dhw_in(d.vr, "dhw"), b.vol_out("hwd")
        arena.poison()
        sd.cross_arms_pair(l, r, TAU, dist, sl, sr)
        res = {}
        res["reference order x2"], _ = sd.cbca(ref_io[0], ref_io[1], sl, 2, dist, hip.MCCNN_CBCA_REFERENCE_ORDER)
        res["separable x1"], _ = sd.cbca(sep_io[0], sep_io[1], sl, 1, dist, hip.MCCNN_CBCA_SEPARABLE)
        res["both views x2 l"], _ = sd.cbca_both_views(both_l[0], both_l[1], sl, sr, 2, dist, hip.MCCNN_SIDE_LEFT)
        res["both views x2 r"], _ = sd.cbca_both_views(both_r[0], both_r[1], sr, sl, 2, dist, hip.MCCNN_SIDE_RIGHT)
        res["hwd"] = sd.dhw_to_hwd(t_in, t_out)
        return res
    ra, _ = run(case, shape, 12)
    t = Tally("plane-major aggregation %s L=%d" % (shape, dist))
    t.bits(ra["reference order x2"], d.agg(2, dist)[0], "mccnn_cbca_iter, reference order")
    al, ar = o.cross_arms(d.L, TAU, dist)[0], o.cross_arms(d.R, TAU, dist)[0]
    R = ppr.clamp_of(dist)
    t.bits(ra["both views x2 l"], finite(ppr.both_views(d.vl, al, ar, 0, R, 2)), "mccnn_cbca_iter_both left")
    t.bits(ra["both views x2 r"], finite(ppr.both_views(d.vr, ar, al, 1, R, 2)), "mccnn_cbca_iter_both right")
    check_vol(t, ra["hwd"], d.vr, D, "mccnn_dhw_to_hwd")
    mean = fk.region_mean64(d.vl, al)
    bound = fk.separable_tolerance(mean, np.abs(d.vl).max()) if dist <= 14 else fk.tile_kernel_bound(d.vl, al)
    err = np.abs(ra["separable x1"].astype(np.float64) - mean)
    t.check(bool((err <= bound).all()), "mccnn_cbca_iter, separable: %d entries outside the stated bound (worst %g)" % (
        int((err > bound).sum()), float((err - bound).max())))
    t.settle(floor=5)


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=_ids(SMALL_SHAPES))
def test_post_processing_red_zones(sd, shape):
    """mccnn_wta, mccnn_subpixel, mccnn_lr_status, mccnn_interpolate, mccnn_interpolate_ex, mccnn_median (5x5 and 3x7),
    mccnn_bilateral on maps and plane-major volumes between red zones, against the oracle (interpolate_ex against
    tests/paper_rules_reference.py)."""
    import oracle as o
    import paper_rules_reference as ppr
    H, W, D = shape
    d, m = data(shape), map_data(shape)
    rng = np.random.default_rng(H + W)
    dl = m.wta.copy()
    dr = np.where(rng.random((H, W)) < 0.6, dl, np.floor(rng.random((H, W)) * D).astype(np.float32)).astype(np.float32)
    status = o.lr_status(dl, dr, D)
    assert {0, 1, 2} <= set(np.unique(status).tolist()) or H * W < 100
    sub_in = m.map

    def case(arena):
        b = Bufs(arena, sd, shape)
        img = b.image(d.L, "image")
        vol = b.dhw_in(m.vol, "vol")
        tdl, tdr, tsub = b.map_in(dl, "dl"), b.map_in(dr, "dr"), b.map_in(sub_in, "sub_in")
        tst = b.map_in(status, "status_in")
        outs = {n: b.map_out(n) for n in ("wta", "subpixel", "interpolate", "interpolate_ex", "median5x5", "median3x7",
                                          "bilateral")}
        st = b.map_out("lr_status", torch.int32)
        arena.poison()
        sd.wta(vol, out=outs["wta"])
        sd.subpixel(tsub, vol, out=outs["subpixel"])
        sd.lr_status(tdl, tdr, D, out=st)
        sd.interpolate(tdl, tst, out=outs["interpolate"])
        sd.interpolate(tdl, tst, out=outs["interpolate_ex"], directions=16, occlusion_from_left=True)
        sd.median(tdl, 5, 5, out=outs["median5x5"])
        sd.median(tdl, 3, 7, out=outs["median3x7"])
        sd.bilateral(img, tdl, 5, 5, 0, 6, 2, out=outs["bilateral"])
        outs["lr_status"] = st
        return outs
    ra, _ = run(case, shape, 3)
    t = Tally("post-processing %s" % (shape,))
    t.bits(ra["wta"], m.wta, "mccnn_wta")
    t.bits(ra["subpixel"], m.sub, "mccnn_subpixel")
    t.equal(ra["lr_status"], status, "mccnn_lr_status")
    t.bits(ra["interpolate"], finite(o.interpolation(dl, dr, D)), "mccnn_interpolate")
    t.bits(ra["interpolate_ex"], finite(ppr.interpolate_ex(dl, status, 16, True)), "mccnn_interpolate_ex")
    t.bits(ra["median5x5"], finite(o.median_filter(dl, 5, 5)), "mccnn_median 5x5")
    t.bits(ra["median3x7"], finite(o.median_filter(dl, 3, 7)), "mccnn_median 3x7")
    t.bits(ra["bilateral"], finite(o.bilateral_filter(d.L, dl, 5, 5, 0, 6, 2)), "mccnn_bilateral")
    t.settle(floor=8)


# ======================================================================================================================
# C: the library-private buffers must be 16-byte aligned - refused on the host, nothing launched
# ======================================================================================================================
def test_misaligned_private_buffers_are_refused_before_any_launch(sd):
    """Support planes, aggregation programs and SGM flag planes at a 4-byte-aligned base: MCCNN_E_INVALID (the scratch /
    flag buffer: MCCNN_E_SCRATCH, as mccnn_speckle_filter answers), and every output keeps its fill."""
    import _hipabi as hip
    shape = (5, 12, 6)
    H, W, D = shape
    d, s = data(shape), sgm_data(shape)
    arena = A.Arena(arena_bytes(shape, 12), "cuda", fill="A")
    b = Bufs(arena, sd, shape)
    l, r = b.image(d.L, "left"), b.image(d.R, "right")
    good_l, good_r = b.support("support_l"), b.support("support_r")
    bad_l, bad_r = b.support("support_l_odd", mod=4), b.support("support_r_odd", mod=8)
    good_p, bad_p = b.progs(), b.progs("prog_odd", mod=12)
    good_f, bad_f = b.flags("flags"), b.flags("flags_odd", mod=4)
    vin, vin2 = b.vol_in(d.vl, "in"), b.vol_in(d.vr, "in2")
    out, out2 = b.vol_out("out"), b.vol_out("out2")
    pin, pout = b.dhw_in(d.vl, "dhw_in"), b.dhw_out("dhw_out")
    dl, dr = b.map_out("dl"), b.map_out("dr")
    arena.poison()
    sd.cross_arms_pair(l, r, TAU, 14, good_l, good_r)
    sd.cbca_prog_build_pair(good_l, good_r, D, 14, good_p, "both")
    lib, st, P = b.lib, hip.stream(), hip.ptr
    p1h, p1v, p2, q1, q2, thr = sd._sgm_penalties(*s.hp)
    n1, side1, vols1 = sd._sgm_arrays([0], [out])
    _, _, src1, acc1 = sd._sgm_arrays([0], [vin], [out])
    _, _, dsrc1, ddst1 = sd._sgm_arrays([0], [pin], [out])
    INV, SCR = hip.MCCNN_E_INVALID, hip.MCCNN_E_SCRATCH
    calls = [
        ("mccnn_cross_arms", INV, lambda: lib.mccnn_cross_arms(P(l), H, W, TAU, 14, P(bad_l), st)),
        ("mccnn_cross_arms_pair", INV, lambda: lib.mccnn_cross_arms_pair(P(l), P(r), H, W, TAU, 14, P(good_l), P(bad_r), st)),
        ("mccnn_cbca_iter_hwd", INV, lambda: lib.mccnn_cbca_iter_hwd(P(vin), P(out), P(bad_l), D, H, W, 14, st)),
        ("mccnn_cbca_iter_hwd_pair", INV, lambda: lib.mccnn_cbca_iter_hwd_pair(P(vin), P(out), P(good_l), P(vin2), P(out2),
                                                                             P(bad_r), D, H, W, 14, st)),
        ("mccnn_cbca_iter_hwd_pair_wta", INV, lambda: lib.mccnn_cbca_iter_hwd_pair_wta(
            P(vin), P(out), P(bad_l), P(vin2), P(out2), P(good_r), D, H, W, 14, P(dl), P(dr), 1, st)),
        ("mccnn_cbca_iter_hwd_long", INV, lambda: lib.mccnn_cbca_iter_hwd_long(P(vin), P(out), P(bad_l), D, H, W, 14, st)),
        ("mccnn_cbca_iter_hwd_long_pair", INV, lambda: lib.mccnn_cbca_iter_hwd_long_pair(
            P(vin), P(out), P(good_l), P(vin2), P(out2), P(bad_r), D, H, W, 14, st)),
        ("mccnn_cbca_iter", INV, lambda: lib.mccnn_cbca_iter(P(pin), P(pout), P(bad_l), D, H, W, 14, 1, st)),
        ("mccnn_cbca_iter_both", INV, lambda: lib.mccnn_cbca_iter_both(P(pin), P(pout), P(good_l), P(bad_r), D, H, W, 14, 0, st)),
        ("mccnn_cbca_prog_build_pair (support)", INV, lambda: lib.mccnn_cbca_prog_build_pair(
            P(bad_l), P(good_r), D, H, W, 14, P(good_p[0]), P(good_p[1]), st)),
    ]
    for name in ("mccnn_cbca_prog_build_pair", "mccnn_cbca_prog_build_skip_pair", "mccnn_cbca_prog_build_both_pair"):
        calls.append((name, INV, lambda name=name: getattr(lib, name)(P(good_l), P(good_r), D, H, W, 14, P(good_p[0]),
                                                                      P(bad_p[1]), st)))
    for name in ("mccnn_cbca_iter_prog", "mccnn_cbca_iter_prog_skip", "mccnn_cbca_iter_prog_refresh"):
        calls.append((name, INV, lambda name=name: getattr(lib, name)(P(vin), P(out), P(good_l), P(bad_p[0]), D, H, W, 14, st)))
    for name in ("mccnn_cbca_iter_prog_pair", "mccnn_cbca_iter_prog_pair_skip", "mccnn_cbca_iter_prog_pair_refresh"):
        calls.append((name, INV, lambda name=name: getattr(lib, name)(P(vin), P(out), P(good_l), P(good_p[0]), P(vin2), P(out2),
                                                                      P(good_r), P(bad_p[1]), D, H, W, 14, st)))
    calls += [
        ("mccnn_cbca_iter_prog_pair_wta", INV, lambda: lib.mccnn_cbca_iter_prog_pair_wta(
            P(vin), P(out), P(good_l), P(bad_p[0]), P(vin2), P(out2), P(good_r), P(good_p[1]), D, H, W, 14, P(dl), P(dr), 1, st)),
        ("mccnn_sgm_flags", SCR, lambda: lib.mccnn_sgm_flags(P(l), P(r), D, H, W, 0, 1, thr, P(bad_f), bad_f.numel(), st)),
        ("mccnn_sgm_pass", SCR, lambda: lib.mccnn_sgm_pass(P(l), P(r), vols1, side1, 1, D, H, W, 0, 1, p1h, p2, q1, q2, thr,
                                                         P(bad_f), bad_f.numel(), st)),
        ("mccnn_sgm_pass_flagged", SCR, lambda: lib.mccnn_sgm_pass_flagged(vols1, side1, 1, D, H, W, 0, 1, p1h, p2, q1, q2,
                                                                         P(bad_f), bad_f.numel(), st)),
        ("mccnn_sgm_pass_accumulate", SCR, lambda: lib.mccnn_sgm_pass_accumulate(src1, acc1, side1, 1, D, H, W, 0, 1, p1h, p2,
                                                                               q1, q2, 0, P(bad_f), bad_f.numel(), st)),
        ("mccnn_sgm_first_pass", SCR, lambda: lib.mccnn_sgm_first_pass(P(l), P(r), dsrc1, ddst1, side1, 1, D, H, W, p1h, p2, q1,
                                                                     q2, thr, P(bad_f), bad_f.numel(), st)),
    ]
    t = Tally("refusals")
    for name, code, call in calls:
        rc = call()
        t.check(rc == code, "%s answered %d, not %d" % (name, rc, code))
        t.check(b"16-byte aligned" in lib.mccnn_last_error_string(), "%s: %r" % (name, lib.mccnn_last_error_string()))
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("out2", out2), ("dhw_out", pout), ("dl", dl), ("dr", dr), ("flags_odd", bad_f),
                      ("prog_odd_l", bad_p[0]), ("prog_odd_r", bad_p[1])):
        t.check(arena.holds_fill(buf), "%s was written by a refused call" % name)
    for name in ("support_l_odd", "support_r_odd"):
        e = next(e for e in arena.entries if e.name == name)
        t.check(arena.holds_fill(e.tensor), "%s was written by a refused call" % name)
    arena.check()
    # the same buffers, aligned, are accepted (the refusals above are about the address and nothing else)
    assert lib.mccnn_cbca_iter_prog(P(vin), P(out), P(good_l), P(good_p[0]), D, H, W, 14, st) == 0
    assert lib.mccnn_sgm_flags(P(l), P(r), D, H, W, 0, 1, thr, P(good_f), good_f.numel(), st) == 0
    torch.cuda.synchronize()
    arena.check()
    t.settle(floor=2 * len(calls) + 10)


# ======================================================================================================================
# D: the matcher on a dirty workspace
# ======================================================================================================================
MATCHERS = {
    "default": (dict(), None, "prog"),
    "hwd": (dict(cbca_kernel="hwd"), None, "hwd"),
    "free_chains_off": (dict(free_chains=False), None, "prog"),
    "two_chains_off": (dict(two_chains=False), None, "prog"),
    "plane_major": (dict(layout="plane_major"), None, "plane_major"),
    "hwd_long": (dict(), dict(cbca_distance=28), "hwd_long"),
}
PAIRS = [(24, 70, 65), (24, 140, 130)]
_PAIR_CASES = {}


def _pair_case(env, shape, hp):
    import synthetic
    key = (shape, tuple(sorted((hp or {}).items())))
    if key not in _PAIR_CASES:
        H, W, D = shape
        L, R = synthetic.make_pair(H, W, D, seed=0)[:2]
        _PAIR_CASES[key] = _case(env, L, R, D, hp)
        assert np.isfinite(_PAIR_CASES[key].want).all()
    return _PAIR_CASES[key]


@pytest.mark.parametrize("route", sorted(MATCHERS))
def test_matcher_on_a_dirty_workspace(env, route):
    """StereoMatcher.workspace() hands out torch.empty volume buffers that serve both layouts: in production their pads
    hold stale costs.  Here they hold fill A, then fill B, in front of match(), match() again and two match_graph() calls:
    every map equals the others and the oracle's (on the GPU's own features), and under keep={} every stage does."""
    kw, hp, want_route = MATCHERS[route]
    sdm = env["sd"]
    m = sdm.StereoMatcher(env["net"], hp=hp, on_saturation="raise", **kw)
    t = Tally("dirty workspace, " + route)
    try:
        for shape in PAIRS:
            H, W, D = shape
            case = _pair_case(env, shape, hp)
            assert m.route(H, W, D) == want_route
            ws = m.workspace(H, W, D)
            what = "%s %dx%dx%d" % (route, W, H, D)

            def dirty(fill):
                torch.cuda.synchronize()
                for v in ws["vol"]:
                    A.fill_tensor(v, fill)
            dirty("A")
            maps = [("match() on fill A", m.match(case.l, case.r, D).cpu().numpy())]
            dirty("B")
            maps.append(("match() on fill B", m.match(case.l, case.r, D).cpu().numpy()))
            dirty("A")
            maps.append(("first match_graph() after a refill", m.match_graph(case.l, case.r, D).clone().cpu().numpy()))
            assert m.workspace(H, W, D) is ws
            maps.append(("second match_graph()", m.match_graph(case.l, case.r, D).clone().cpu().numpy()))
            for name, got in maps:
                t.bits(got, case.want, "%s: %s against the oracle" % (what, name))
                t.bits(got, maps[0][1], "%s: %s against the first map" % (what, name))
            dirty("B")
            keep = {}
            got = m.match(case.l, case.r, D, keep=keep).cpu().numpy()
            t.bits(got, case.want, what + ": keep={} map")
            for stage, v in stagewise(keep, case.L, case.R, D, env["o"], hp=m.hp, features=(case.fl, case.fr)).items():
                t.check(v == 0.0, "%s, keep={}: %s differs from the oracle (%g)" % (what, stage, v))
    finally:
        torch.cuda.synchronize()
        m._graphs, m._ws = {}, {}
        m._side = m._right = m._library_twin = None
        torch.cuda.synchronize()
    t.settle(floor=2 * (8 + 1 + 8))
