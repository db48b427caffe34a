"""CPU: what the confidence measures promise without a GPU - every argument refusal of mccnn_confidence_hwd /
mccnn_confidence (validation runs before any HIP call), confidence_mask, properties of the restatement
(tests/confidence_reference.py) on the reference's own golden outputs."""
import ctypes
import os

import numpy as np
import pytest

import confidence_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2


def test_argument_refusals():
    import _hipabi
    lib = _hipabi.load()
    vol = ctypes.c_void_p(0x100000)           # never dereferenced: every call below is refused before any HIP call
    out = ctypes.c_void_p(0x900000)
    right = ctypes.c_void_p(0x500000)

    def msg():
        return lib.mccnn_last_error_string()

    for fn, who in ((lib.mccnn_confidence_hwd, b"mccnn_confidence_hwd"), (lib.mccnn_confidence, b"mccnn_confidence")):
        assert fn(None, right, 8, 4, 6, 15, out, None) == E_INVALID and b"null pointer" in msg() and who in msg()
        assert fn(vol, right, 8, 4, 6, 15, None, None) == E_INVALID and b"null pointer" in msg()
        for D in (1, 0, -3):
            assert fn(vol, right, D, 4, 6, 15, out, None) == E_INVALID and b"two disparities" in msg()
        for H, W in ((0, 6), (4, 0), (-1, 6), (4, -1)):
            assert fn(vol, right, 8, H, W, 15, out, None) == E_INVALID and b"non-positive" in msg()
        for measures in (0, 16, 17, 32, 0x80000000):
            assert fn(vol, right, 8, 4, 6, measures, out, None) == E_INVALID and b"measures" in msg()
        for measures in (8, 9, 15):
            assert fn(vol, None, 8, 4, 6, measures, out, None) == E_INVALID and b"disp_right" in msg()
        plane = 4 * 6 * 4
        for k, measures in ((1, 1), (2, 3), (4, 15)):
            for r in (out.value, out.value + 4, out.value + k * plane - 4, out.value - plane + 4):
                assert fn(vol, ctypes.c_void_p(r), 8, 4, 6, measures, out, None) == E_INVALID and b"overlaps" in msg()
    assert lib.mccnn_confidence_hwd(vol, right, 1025, 4, 6, 15, out, None) == E_UNSUPPORTED and b"1024" in msg()
    assert lib.mccnn_confidence_hwd(vol, None, 4096, 4, 6, 7, out, None) == E_UNSUPPORTED


def test_confidence_mask():
    import stereo_device as sd
    assert sd.CONFIDENCE_MEASURES == ("msm", "mmn", "cur", "lrc") == ref.NAMES
    assert [sd.confidence_mask((n,)) for n in sd.CONFIDENCE_MEASURES] == [1, 2, 4, 8]
    assert sd.confidence_mask(sd.CONFIDENCE_MEASURES) == 15
    assert sd.confidence_mask(["lrc", "msm"]) == 9 and sd.confidence_mask("cur") == 4
    assert sd.confidence_names(("lrc", "msm")) == ("msm", "lrc") and sd.confidence_names(6) == ("mmn", "cur")
    for bad in ((), ("pkr",), ("msm", "msm"), ("MSM",), ""):
        with pytest.raises(ValueError):
            sd.confidence_mask(bad)


def test_header_states_the_measures():
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    import _hipabi
    for name, bit in (("MSM", 1), ("MMN", 2), ("CUR", 4), ("LRC", 8)):
        assert "#define MCCNN_CONF_%s %du" % (name, bit) in text
        assert getattr(_hipabi, "MCCNN_CONF_" + name) == bit == ref.BITS[name.lower()]


@pytest.fixture(scope="module")
def golden_planes(golden_cases):
    """Per golden pair: (name, g, planes [4,H,W], d1) of the reference's final left volume and right map."""
    return [(name, g) + ref.confidence(g["cbca2_l"], g["wta_r"], 15) for name, g in golden_cases]


def _scored(g, planes):
    """A bad / region pair for a golden case: the raw left map against the true disparity, error above one pixel."""
    err = np.abs(g["wta_l"] - g["true_disp"].astype(np.float32))
    region = np.ones(err.shape, bool)
    region[::5, ::3] = False
    return err > 1.0, region


def test_restatement_on_golden_pairs(golden_planes):
    assert len(golden_planes) == 4
    for name, g, planes, d1 in golden_planes:
        assert np.array_equal(d1.astype(np.float32), g["wta_l"]), name
        assert planes.shape == (4,) + g["wta_l"].shape and planes.dtype == np.float32
        assert np.isfinite(planes[:3]).all() and (planes[1] >= 0).all(), name
        assert ((planes[3] <= 0) | np.isnan(planes[3])).all()
        for mask in (1, 2, 4, 8, 5, 10):                      # fewer measures: the same planes, in bit order
            few, _ = ref.confidence(g["cbca2_l"], g["wta_r"], mask)
            want = np.stack([planes[ref.plane_index(15, n)] for n in ref.NAMES if mask & ref.BITS[n]])
            assert np.array_equal(few.view(np.uint32), want.view(np.uint32)), (name, mask)


def test_sparsification_properties(golden_planes):
    for name, g, planes, _ in golden_planes:
        bad, region = _scored(g, planes)
        n, e = int(region.sum()), int((bad & region).sum())
        assert 0 < e < n
        closed = sum((k - (n - e)) / k for k in range(n - e + 1, n + 1)) / n
        rng = np.random.default_rng(n)
        for i, measure in enumerate(ref.NAMES):
            conf = planes[i].copy()
            conf.reshape(-1)[::7] = np.nan                                     # NaN counts as -inf
            s = ref.sparsification(conf, bad, region)
            assert s["n"] == n and s["e"] == e
            assert s["auc_optimal"] <= s["auc"] <= 1.0, (name, measure)
            assert abs(s["auc_optimal"] - closed) <= n * 2.0 ** -52
            # a permutation of the pixels that keeps the index order within ties: sort the pixels by a random key per
            # DISTINCT confidence value, stably - equal confidences stay in their order, everything else moves
            flat = np.where(np.isnan(conf), -np.inf, conf).reshape(-1)
            values, inverse = np.unique(flat, return_inverse=True)
            perm = np.argsort(rng.permutation(values.size)[inverse], kind="stable")
            assert not np.array_equal(perm, np.arange(perm.size))
            t = ref.sparsification(conf.reshape(-1)[perm], bad.reshape(-1)[perm], region.reshape(-1)[perm])
            assert t == s, (name, measure)
        # the oracle ordering (bad pixels last) reaches the optimum; the opposite ordering is the worst
        oracle = ref.sparsification(np.where(bad, 0.0, 1.0).astype(np.float32), bad, region)
        assert abs(oracle["auc"] - oracle["auc_optimal"]) <= n * 2.0 ** -52
    empty = ref.sparsification(planes[0], bad, np.zeros_like(region))
    assert empty["n"] == 0 and empty["e"] == 0 and np.isnan(empty["auc"]) and np.isnan(empty["auc_optimal"])



def test_match_help_lists_the_flag():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--confidence" in out.stdout and "--eval_auc_threshold" in out.stdout


def test_confidence_flag_parsing():
    import match
    assert match.parse_confidence(None) == ()
    assert match.parse_confidence("lrc, mmn") == ("mmn", "lrc") and match.parse_confidence("msm,mmn,cur,lrc") == ref.NAMES
    assert match.CONFIDENCE_MEASURES == ref.NAMES
    for bad in ("", "pkr", "mmn,mmn", ","):
        with pytest.raises(ValueError):
            match.parse_confidence(bad)
