"""CPU: the host side of the metric outputs - the calibration record and its two text forms, the properties of the NumPy
restatement (tests/reproject_reference.py), the PLY writer, the refusals of the three C entry points (before any launch,
so they need no device), match.py's options, StereoMatcher(geometry=...) and the PairResult record with its new fields."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import reproject_reference as ref

CALIB = (3997.684, 3990.25, 1176.728, 1011.728, 193.001, 131.111)


# ---- the calibration ---------------------------------------------------------------------------------------------------
def test_from_middlebury_reads_by_key_in_any_order(tmp_path):
    from calibration import Calibration
    lines = ["cam0=[3997.684 0 1176.728; 0 3990.25 1011.728; 0 0 1]", "cam1=[3997.684 0 1307.839; 0 3997.684 1011.728; 0 0 1]",
             "doffs=131.111", "baseline=193.001", "width=2964", "height=1988", "ndisp=280", "isint=0"]
    want = Calibration(*CALIB)
    for k, order in enumerate(itertools.islice(itertools.permutations(lines), 0, 5040 * 8, 1999)):
        p = tmp_path / ("calib%d.txt" % k)
        p.write_text("\n".join(order) + "\n")
        assert Calibration.from_middlebury(str(p)) == want
    assert want.fx != want.fy
    p = tmp_path / "nodoffs.txt"
    p.write_text("baseline=100\ncam0=[5 0 2; 0 6 3; 0 0 1]\n")
    assert Calibration.from_middlebury(str(p)) == Calibration(5, 6, 2, 3, 100, 0)


@pytest.mark.parametrize("missing", ["cam0", "baseline"])
def test_from_middlebury_names_the_missing_key_and_the_file(tmp_path, missing):
    from calibration import Calibration
    lines = dict(cam0="cam0=[5 0 2; 0 6 3; 0 0 1]", baseline="baseline=100", doffs="doffs=1")
    del lines[missing]
    p = tmp_path / "calib.txt"
    p.write_text("\n".join(lines.values()) + "\n")
    with pytest.raises(ValueError) as e:
        Calibration.from_middlebury(str(p))
    assert missing in str(e.value) and str(p) in str(e.value)


def test_the_calib_text_of_the_cli_tests(tmp_path):
    import util
    from calibration import Calibration
    p = tmp_path / "calib.txt"
    p.write_text("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                 "width=64\nheight=48\nndisp=16\nisint=0\nvmin=0\nvmax=16\ndyavg=0\ndymax=0\n")
    assert tuple(Calibration.from_middlebury(str(p))) == (1, 1, 0, 0, 100, 0)
    assert tuple(util.parseCalib(str(p))) == (48, 64, 16)


def test_parse_round_trip_and_refusals():
    from calibration import Calibration
    c = Calibration(*CALIB)
    assert Calibration.parse(c.describe()) == c and Calibration.parse(c) is c and Calibration.parse(CALIB) == c
    assert Calibration.parse("1,2,3,4,5") == Calibration(1, 2, 3, 4, 5, 0.0)
    assert Calibration.parse(" 1, 2 ,3,4,5,-6.5 ").doffs == -6.5
    for bad in ("", "1,2,3,4", "1,2,3,4,5,6,7", "1,2,x,4,5", "0,2,3,4,5", "1,-2,3,4,5", "1,2,3,4,0", "1,2,nan,4,5",
                "inf,2,3,4,5", "1,2,3,4,5,inf"):
        with pytest.raises(ValueError):
            Calibration.parse(bad)
    fx, fy, cx, cy, fb, doffs = c.scalars()
    assert fb == float(np.float32(CALIB[0] * CALIB[4])) and fx == float(np.float32(CALIB[0]))
    assert all(v == float(np.float32(v)) for v in (fx, fy, cx, cy, fb, doffs))
    assert tuple(float(v) for v in ref.scalars(c)) == c.scalars()


def test_calibration_imports_neither_torch_nor_the_gpu_library():
    import subprocess
    import sys
    import os
    from conftest import ROOT
    code = "import sys, calibration, pair_result; assert 'torch' not in sys.modules and '_hipabi' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.join(ROOT, "mc-cnn-python_amd", "src"))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("doffs", [0.0, 12.5, -3.0])
def test_depth_is_strictly_decreasing_in_d_where_defined(doffs):
    d = np.linspace(max(0.0, -doffs) + 0.25, 900.0, 4001).astype(np.float32)[None, :]
    z = ref.depth(d, CALIB[:5] + (doffs,))[0]
    assert z.dtype == np.float32 and np.isfinite(z).all() and (np.diff(z.astype(np.float64)) < 0).all()


def test_points_project_back_to_their_pixels():
    H, W = 37, 130
    m = ref.ramp(H, W, 3.0, 250.0)
    m[::5, ::7] = np.inf
    for calib in (CALIB, (520.9, 521.0, 64.5, 18.25, 0.16, 0.0)):
        pts = ref.points(m, calib)
        pix = pts[:, 3].copy().view(np.uint32)
        assert np.array_equal(pix, np.flatnonzero(np.isfinite(m)).astype(np.uint32)), "raster order, dropped pixels left out"
        fx, fy, cx, cy = (np.float64(v) for v in ref.scalars(calib)[:4])
        x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
        assert np.abs(fx * x / z + cx - pix % W).max() < 1e-3 and np.abs(fy * y / z + cy - pix // W).max() < 1e-3


@pytest.mark.parametrize("doffs", [0.0, 12.5, -3.0])
def test_every_special_value_gives_inf_and_no_point(doffs):
    d = np.float32(doffs)
    never = np.array([[np.nan, np.inf, -np.inf, -d, np.nextafter(-d, np.float32(-np.inf), dtype=np.float32), -3e38]], np.float32)
    calib = CALIB[:5] + (doffs,)
    z = ref.depth(never, calib)
    assert np.array_equal(ref.bits(z), np.full(never.shape, 0x7F800000, np.uint32))
    assert ref.points(never, calib).shape == (0, 4)
    # -0.0 is an ordinary zero
    zeros = ref.depth(np.array([[-0.0, 0.0]], np.float32), calib)
    assert ref.bits(zeros)[0, 0] == ref.bits(zeros)[0, 1] and np.isfinite(zeros[0, 0]) == (doffs > 0)
    # max_depth: inclusive, and +inf keeps every finite Z
    m = ref.ramp(4, 9, 20.0, 40.0)
    zz = np.sort(ref.depth(m, calib).reshape(-1))
    assert ref.points(m, calib).shape[0] == 36
    assert ref.points(m, calib, float(zz[10])).shape[0] == 11
    assert ref.points(m, calib, -1.0).shape[0] == 0


# ---- the PLY writer ----------------------------------------------------------------------------------------------------
def test_ply_round_trip_and_the_empty_cloud(tmp_path):
    from calibration import point_pixels, read_ply, write_ply
    m = ref.ramp(6, 11, 2.0, 30.0)
    m[2, 3] = np.inf
    records = ref.points(m, CALIB)
    grey = (np.arange(66) * 7 % 256).astype(np.uint8)
    pix = point_pixels(records)
    assert pix.dtype == np.uint32 and pix.size == 65 and 25 not in pix
    p = str(tmp_path / "points.ply")
    write_ply(p, records, grey[pix])
    blob = open(p, "rb").read()
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 65\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar intensity\nend_header\n")
    assert blob.startswith(head) and len(blob) == len(head) + 65 * 13
    xyz, intensity = read_ply(p)
    assert np.array_equal(ref.bits(xyz), ref.bits(records[:, :3])) and np.array_equal(intensity, grey[pix])
    write_ply(p, np.zeros((0, 4), np.float32), np.zeros((0,), np.uint8))
    xyz, intensity = read_ply(p)
    assert xyz.shape == (0, 3) and intensity.shape == (0,) and b"element vertex 0\n" in open(p, "rb").read()


# ---- the C entry points refuse before they launch ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import _hipabi
    _hipabi.load()
    return _hipabi


P = ctypes.c_void_p
MAP, OUT, COUNT, SCRATCH = 0x100000, 0x200000, 0x300000, 0x400000       # never dereferenced: every call is refused


def _depth(hip, **kw):
    a = dict(map=P(MAP), H=4, W=5, fb=100.0, doffs=0.0, depth=P(OUT))
    a.update(kw)
    rc = hip.load().mccnn_depth(a["map"], a["H"], a["W"], a["fb"], a["doffs"], a["depth"], None)
    return rc, hip.load().mccnn_last_error_string().decode()


def _points(hip, **kw):
    a = dict(map=P(MAP), H=4, W=5, fx=1.0, fy=1.0, cx=0.0, cy=0.0, fb=100.0, doffs=0.0, max_depth=math.inf, points=P(OUT),
             n_points=P(COUNT), scratch=P(SCRATCH), scratch_bytes=16)
    a.update(kw)
    rc = hip.load().mccnn_reproject_points(a["map"], a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["fb"], a["doffs"],
                                           a["max_depth"], a["points"], a["n_points"], a["scratch"], a["scratch_bytes"], None)
    return rc, hip.load().mccnn_last_error_string().decode()


def test_entry_refuses_null_pointers(hip):
    for name in ("map", "depth"):
        rc, msg = _depth(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "mccnn_depth: null pointer" in msg, (name, rc, msg)
    for name in ("map", "points", "n_points", "scratch"):
        rc, msg = _points(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "mccnn_reproject_points: null pointer" in msg, (name, rc, msg)


@pytest.mark.parametrize("size", [dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)])
def test_entry_refuses_non_positive_sizes(hip, size):
    for call in (_depth, _points):
        rc, msg = call(hip, **size)
        assert rc == hip.MCCNN_E_INVALID and "non-positive size" in msg, (rc, msg)
    assert hip.load().mccnn_points_scratch_bytes(size.get("H", 4), size.get("W", 5)) == 0


def test_entry_refuses_a_short_or_misaligned_scratch_and_names_the_bytes(hip):
    need = hip.load().mccnn_points_scratch_bytes(1025, 1030)
    assert need == 4144 and hip.load().mccnn_points_scratch_bytes(4, 5) == 16
    rc, msg = _points(hip, H=1025, W=1030, scratch_bytes=need - 1)
    assert rc == hip.MCCNN_E_SCRATCH and "%d bytes" % (need - 1) in msg and "= %d" % need in msg, (rc, msg)
    rc, msg = _points(hip, scratch=P(SCRATCH + 4))
    assert rc == hip.MCCNN_E_SCRATCH and "scratch must be 16-byte aligned" in msg, (rc, msg)
    rc, msg = _points(hip, points=P(OUT + 4))
    assert rc == hip.MCCNN_E_INVALID and "points must be 16-byte aligned" in msg, (rc, msg)
    assert hip.load().mccnn_points_scratch_bytes(46341, 46341) == 0       # beyond 2^31 - 1 pixels
    rc, msg = _points(hip, H=46341, W=46341, scratch_bytes=1 << 30)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "46341 x 46341" in msg, (rc, msg)


@pytest.mark.parametrize("value", [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_entry_refuses_focal_lengths_and_fb_that_are_not_finite_and_positive(hip, value):
    rc, msg = _depth(hip, fb=value)
    assert rc == hip.MCCNN_E_INVALID and "mccnn_depth: fb=" in msg, (rc, msg)
    for name in ("fx", "fy", "fb"):
        rc, msg = _points(hip, **{name: value})
        assert rc == hip.MCCNN_E_INVALID and "mccnn_reproject_points: %s=" % name in msg, (name, rc, msg)


def test_entry_refuses_a_nan_max_depth_and_non_finite_offsets(hip):
    rc, msg = _points(hip, max_depth=math.nan)
    assert rc == hip.MCCNN_E_INVALID and "max_depth is NaN" in msg, (rc, msg)
    for value in (math.nan, math.inf):
        rc, msg = _points(hip, doffs=value)
        assert rc == hip.MCCNN_E_INVALID and "doffs=" in msg, (rc, msg)
        rc, msg = _depth(hip, doffs=value)
        assert rc == hip.MCCNN_E_INVALID and "doffs=" in msg, (rc, msg)
        rc, msg = _points(hip, cx=value)
        assert rc == hip.MCCNN_E_INVALID and "cx=" in msg, (rc, msg)
    # (a negative or infinite max_depth is a value like any other: the call gets as far as the launch)


def test_entry_refuses_overlapping_buffers(hip):
    rc, msg = _depth(hip, depth=P(MAP + 16))
    assert rc == hip.MCCNN_E_INVALID and "depth overlaps map" in msg, (rc, msg)
    rc, msg = _points(hip, points=P(MAP + 16))
    assert rc == hip.MCCNN_E_INVALID and "output overlaps map" in msg, (rc, msg)
    rc, msg = _points(hip, scratch=P(OUT + 64))
    assert rc == hip.MCCNN_E_INVALID and "scratch overlaps" in msg, (rc, msg)


def test_abi_version_is_unchanged_and_the_symbols_are_in_the_table(hip):
    assert hip.load().mccnn_version() == 7 == hip.MCCNN_ABI_VERSION
    for name in ("mccnn_depth", "mccnn_points_scratch_bytes", "mccnn_reproject_points"):
        assert name in hip.SIGNATURES


# ---- match.py -----------------------------------------------------------------------------------------------------------
BASE = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]


def test_match_parser_has_the_options_and_they_are_off():
    import match
    a = match.parser.parse_args(BASE)
    assert a.depth is False and a.point_cloud is False and a.max_depth is None and a.calib is None
    a = match.parser.parse_args(BASE + ["--depth", "--point_cloud", "--max_depth", "5000", "--calib", "1,2,3,4,5"])
    assert a.depth and a.point_cloud and a.max_depth == 5000.0 and a.calib == "1,2,3,4,5"


@pytest.mark.parametrize("extra,reason", [
    (["--depth", "--dataset", "kitti2015"], "--depth is not available with --dataset kitti2015: the development kit's calibration"),
    (["--point_cloud", "--dataset", "kitti2012"], "--point_cloud is not available with --dataset kitti2012"),
    (["--max_depth", "10"], "--max_depth goes with --point_cloud"),
    (["--depth", "--max_depth", "10"], "--max_depth goes with --point_cloud"),
    (["--point_cloud", "--max_depth", "nan"], "--max_depth: NaN"),
    (["--calib", "1,2,3,4,5"], "--calib goes with --depth or --point_cloud"),
    (["--depth", "--calib", "1,2,3"], "--calib: expected fx,fy,cx,cy,baseline[,doffs]"),
    (["--depth", "--calib", "0,2,3,4,5"], "--calib: ")])
def test_match_refuses(extra, reason, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + extra)
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert reason in err, err


# ---- the matcher's option ---------------------------------------------------------------------------------------------
class _StubNet(object):
    def supports_split_features(self):
        return True


@pytest.fixture
def sd(monkeypatch):
    import torch
    import stereo_device
    monkeypatch.setattr(stereo_device.hip, "require_device", lambda: torch.device("cpu"))
    return stereo_device


def test_matcher_geometry_option(sd):
    from calibration import Calibration
    H, W, D = 40, 48, 16
    plain = sd.StereoMatcher(_StubNet())
    none = sd.StereoMatcher(_StubNet(), geometry=None)
    assert plain.geometry is None and none.geometry is None and none._geometry_kw() == {}
    assert none.extras == plain.extras
    base = sd.workspace_bytes(H, W, D, plain.pixel_major(), plain.workspace_cbca_kernel(H, W, D))
    assert sd.workspace_bytes(H, W, D, none.pixel_major(), none.workspace_cbca_kernel(H, W, D), **none._geometry_kw()) == base
    scratch = sd.hip.load().mccnn_points_scratch_bytes(H, W)
    m = sd.StereoMatcher(_StubNet(), geometry=dict(calib="1,2,3,4,5", depth=True, points=True, max_depth=7))
    assert m.geometry == dict(calib=Calibration(1, 2, 3, 4, 5), depth=True, points=True, max_depth=7.0)
    grown = sd.workspace_bytes(H, W, D, m.pixel_major(), m.workspace_cbca_kernel(H, W, D), **m._geometry_kw())
    assert grown == base + H * W * 4 + H * W * 16 + scratch + 4
    assert sd.workspace_bytes(H, W, D, m.pixel_major(), m.workspace_cbca_kernel(H, W, D), depth=True) == base + H * W * 4
    m.set_calibration((5, 4, 3, 2, 1, 0.5))
    assert m.geometry["calib"] == Calibration(5, 4, 3, 2, 1, 0.5)
    assert m._graph_key((H, W, D)) != sd.StereoMatcher(_StubNet(), geometry=dict(calib="1,2,3,4,5", depth=True))._graph_key((H, W, D))
    assert plain._graph_key((H, W, D)) == (H, W, D)
    with pytest.raises(ValueError, match="unknown geometry keys"):
        sd.StereoMatcher(_StubNet(), geometry=dict(calib="1,2,3,4,5", depth=True, cloud=True))
    with pytest.raises(ValueError, match="neither depth nor points"):
        sd.StereoMatcher(_StubNet(), geometry=dict(calib="1,2,3,4,5"))
    with pytest.raises(ValueError, match="NaN"):
        sd.StereoMatcher(_StubNet(), geometry=dict(points=True, max_depth=float("nan")))
    with pytest.raises(ValueError):
        sd.StereoMatcher(_StubNet(), geometry=dict(calib="1,2,3", points=True))
    with pytest.raises(ValueError, match="no geometry"):
        plain.set_calibration("1,2,3,4,5")
    # the results a matcher's configuration announces
    only_depth = sd.StereoMatcher(_StubNet(), semi_dense="lr", geometry=dict(depth=True))
    assert only_depth.result_of(("m", "s", "z")) == (("m", None, "s", "z", None, None))
    assert m.result_of(("m", "z", "p", "n")) == ("m", None, None, "z", "p", "n")
    assert plain.result_of("m") == ("m", None, None, None, None, None)


# ---- the record --------------------------------------------------------------------------------------------------------
def test_pair_result_keeps_its_old_constructions():
    from pair_result import PairResult
    assert PairResult("m") == ("m", None, None, None, None, None) and PairResult("m").public() == "m"
    r = PairResult("m", "p", "s")
    assert (r.map, r.planes, r.sparse, r.depth, r.points, r.n_points) == ("m", "p", "s", None, None, None)
    assert r.public() == ("m", "p", "s") and PairResult.decode(r.public(), True, True) == r
    assert PairResult.decode("m", False, False) == PairResult("m")
    assert PairResult(None).map is None and PairResult._fields[:3] == ("map", "planes", "sparse")
    assert PairResult._fields[3:] == ("depth", "points", "n_points")


def test_pair_result_round_trips_every_combination():
    from pair_result import PairResult
    for planes, sparse, depth, points in itertools.product((False, True), repeat=4):
        r = PairResult("m", "p" if planes else None, "s" if sparse else None, "z" if depth else None,
                       "c" if points else None, "n" if points else None)
        pub = r.public()
        if not (planes or sparse or depth or points):
            assert pub == "m"
        else:
            assert isinstance(pub, tuple) and len(pub) == 1 + planes + sparse + depth + 2 * points and pub[0] == "m"
        assert PairResult.decode(pub, planes, sparse, depth, points) == r
        assert r.apply(lambda t: t.upper()) == PairResult(*(t.upper() if t else None for t in r))
        assert r.view(0, False) is r
    both = PairResult(["l", "r"], None, ["ls", "rs"], "z", "c", "n")
    assert both.view(0, True) == PairResult("l", None, "ls", "z", "c", "n")
    assert both.view(1, True) == PairResult("r", None, "rs")
