"""CPU: the paper-faithful SGM stage (four independent directions, averaged; tests/paper_sgm_reference.py) pinned
against the real reference's single-direction volumes in tests/golden/, the argument validation of the five SGM entry
points without a GPU, the command-line flag and the matcher extra, and the reason for having it:
on synthetic pairs the paper's stage beats the reference's sequential composition."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import assert_bits, hp_of
import paper_sgm_reference as ps


def _sgm_hp(hp):
    return [hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]


def test_helper_equals_the_average_of_the_reference_directions(golden_cases):
    """From cbca1_* the helper gives (sgm_right + sgm_left + sgm_up + sgm_bottom) / 4. of the fixtures - volumes the real
    reference produced one direction at a time from that same input - bit for bit, leaves its input alone, and is not
    the sequential result sgm_*."""
    for name, g in golden_cases:
        hp = hp_of(g)
        for side, choice in (("l", "L"), ("r", "R")):
            src = g["cbca1_" + side]
            before = src.copy()
            got = ps.sgm_independent(src, g["left"], g["right"], *_sgm_hp(hp), choice)
            want = ps.average4([g["sgm_%s_%s" % (d, side)] for d in ps.NAMES])
            assert_bits(got, want, "%s %s: helper against the fixtures' average" % (name, side))
            assert_bits(src, before, "%s %s: input modified" % (name, side))
            differ = (got.view(np.uint32) != g["sgm_" + side].view(np.uint32)).mean()
            assert differ > 0.99, "%s %s: only %.4f of the voxels differ from the sequential result" % (name, side, differ)


def test_both_sides_helper_has_the_signature_of_sgm_average(golden_cases):
    name, g = golden_cases[0]
    hp = hp_of(g)
    l, r = ps.SGM_average_independent(g["cbca1_l"], g["cbca1_r"], g["left"], g["right"], *_sgm_hp(hp))
    assert_bits(l, ps.average4([g["sgm_%s_l" % d] for d in ps.NAMES]), name + " left")
    assert_bits(r, ps.average4([g["sgm_%s_r" % d] for d in ps.NAMES]), name + " right")


# ---- the SGM entry points: validation before any launch ------------------------------------------------------------
# the pointer arguments of each entry point, by the names _Args gives them
POINTERS = {
    "mccnn_sgm_pass": ("left", "right", "src", "side", "flags"),
    "mccnn_sgm_flags": ("left", "right", "flags"),
    "mccnn_sgm_pass_flagged": ("src", "side", "flags"),
    "mccnn_sgm_pass_accumulate": ("src", "acc", "side", "flags"),
    "mccnn_sgm_first_pass": ("left", "right", "src", "acc", "side", "flags"),
}
ENTRIES = tuple(POINTERS)
WITH_JOBS = tuple(e for e in ENTRIES if "side" in POINTERS[e])
WITH_DIRECTION = tuple(e for e in ENTRIES if e != "mccnn_sgm_first_pass")


class _Args(object):
    """A valid call of one entry point on fake addresses (nothing is dereferenced before validation ends; every case below
    fails it).  src / acc: the volume lists - the in-place passes have `src` only (their vol_hwd), the first pass reads
    `src` (plane-major) and writes `acc`."""

    def __init__(self, hip, n_jobs=1, D=8, H=4, W=12, entry="mccnn_sgm_pass_accumulate"):
        lib = hip.load()
        self.lib, self.hip, self.entry = lib, hip, entry
        self.D, self.H, self.W, self.n = D, H, W, n_jobs
        vol = H * W * lib.mccnn_hwd_pitch(D) * 4
        self.vol = vol
        base = 0x10000000
        self.src = [base, base + 4 * vol]
        self.acc = [base + 2 * vol, base + 6 * vol]
        self.side = [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT]
        self.r = (0, 1)
        self.mode = hip.MCCNN_SGM_ACC_STORE
        self.images = [0x60000000, 0x68000000]
        self.flags = 0x70000000
        self.flags_bytes = lib.mccnn_sgm_scratch_bytes(H, W, D)

    def call(self, src_null=False, acc_null=False, side_null=False, left_null=False, right_null=False):
        vp2, i2 = ctypes.c_void_p * 2, ctypes.c_int * 2
        src = None if src_null else vp2(*self.src)
        acc = None if acc_null else vp2(*self.acc)
        side = None if side_null else i2(*self.side)
        left = None if left_null else ctypes.c_void_p(self.images[0])
        right = None if right_null else ctypes.c_void_p(self.images[1])
        shape, r, pen = (self.D, self.H, self.W), (self.r[0], self.r[1]), (2.3, 55.9, 4.0, 8.0)
        tail = (ctypes.c_void_p(self.flags), self.flags_bytes, None)
        args = {
            "mccnn_sgm_pass": (left, right, src, side, self.n) + shape + r + pen + (0.08,) + tail,
            "mccnn_sgm_flags": (left, right) + shape + r + (0.08,) + tail,
            "mccnn_sgm_pass_flagged": (src, side, self.n) + shape + r + pen + tail,
            "mccnn_sgm_pass_accumulate": (src, acc, side, self.n) + shape + r + pen + (self.mode,) + tail,
            "mccnn_sgm_first_pass": (left, right, src, acc, side, self.n) + shape + pen + (0.08,) + tail,
        }[self.entry]
        rc = getattr(self.lib, self.entry)(*args)
        return rc, self.lib.mccnn_last_error_string().decode()


@pytest.fixture(scope="module")
def hip():
    import _hipabi
    _hipabi.load()
    return _hipabi


def test_accumulate_refuses_null_pointers(hip):
    for kw in (dict(src_null=True), dict(acc_null=True), dict(side_null=True)):
        rc, msg = _Args(hip).call(**kw)
        assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg, (kw, rc, msg)
    a = _Args(hip)
    a.flags = None
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg
    for which in ("src", "acc"):
        a = _Args(hip, n_jobs=2)
        getattr(a, which)[1] = None
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "null volume" in msg, (which, rc, msg)


def test_accumulate_refuses_overlapping_buffers(hip):
    a = _Args(hip)
    a.acc[0] = a.src[0]                                     # src == acc
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "overlaps" in msg, (rc, msg)
    for shift in (-4, 4):                                   # one float short of disjoint, on either side
        a = _Args(hip)
        a.acc[0] = a.src[0] + shift * (a.vol // 4 - 1)
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "overlaps" in msg, (shift, rc, msg)
    a = _Args(hip, n_jobs=2)                                # the accumulator of one job on the source of the other
    a.acc[1] = a.src[0] + 16
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "overlaps" in msg, (rc, msg)
    a = _Args(hip, n_jobs=2)                                # two jobs into one accumulator
    a.acc[1] = a.acc[0]
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "overlap" in msg, (rc, msg)


def test_accumulate_refuses_unknown_modes(hip):
    for mode in (-1, 3, 100):
        a = _Args(hip)
        a.mode = mode
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "mode=%d" % mode in msg, (mode, rc, msg)
    assert (hip.MCCNN_SGM_ACC_STORE, hip.MCCNN_SGM_ACC_ADD, hip.MCCNN_SGM_ACC_ADD_QUARTER) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    for name, value in (("STORE", 0), ("ADD", 1), ("ADD_QUARTER", 2)):
        assert "#define MCCNN_SGM_ACC_%s %d" % (name, value) in header


def test_accumulate_refuses_disparity_counts_outside_2_to_1024(hip):
    for D in (0, 1, 1025, 4096):
        a = _Args(hip)
        a.D = D
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_UNSUPPORTED and "outside [2,1024]" in msg, (D, rc, msg)


def test_accumulate_refuses_directions_that_are_not_unit_axis_steps(hip):
    for r in ((0, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, -1)):
        a = _Args(hip)
        a.r = r
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "axis-aligned unit step" in msg, (r, rc, msg)


def test_accumulate_refuses_short_flag_planes(hip):
    a = _Args(hip)
    a.flags_bytes -= 1
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_SCRATCH and "scratch" in msg, (rc, msg)


def test_accumulate_refuses_bad_job_counts_and_sides(hip):
    for n in (0, 3):
        a = _Args(hip)
        a.n = n
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "n_jobs" in msg
    a = _Args(hip)
    a.side[0] = 7
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "side" in msg


# the same cases on every entry point (an entry point without the argument leaves the case out)
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_point_refuses_null_pointers(hip, entry):
    for name in POINTERS[entry]:
        a = _Args(hip, entry=entry)
        if name == "flags":
            a.flags = None
            rc, msg = a.call()
        else:
            rc, msg = a.call(**{name + "_null": True})
        assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg and msg.startswith(entry + ":"), (name, rc, msg)
    for which in ("src", "acc"):                             # a null second volume
        if which in POINTERS[entry]:
            a = _Args(hip, n_jobs=2, entry=entry)
            getattr(a, which)[1] = None
            rc, msg = a.call()
            assert rc == hip.MCCNN_E_INVALID and "null volume" in msg, (which, rc, msg)


@pytest.mark.parametrize("entry", WITH_JOBS)
def test_every_entry_point_refuses_bad_job_counts_and_sides(hip, entry):
    for n in (0, 3):
        a = _Args(hip, entry=entry)
        a.n = n
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "n_jobs" in msg, (n, rc, msg)
    a = _Args(hip, entry=entry)
    a.side[0] = 7
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_INVALID and "side" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_point_refuses_disparity_counts_outside_its_range(hip, entry):
    first = entry == "mccnn_sgm_first_pass"                  # one 256-disparity group
    for D in ((0, 1, 257) if first else (0, 1, 1025, 4096)):
        a = _Args(hip, entry=entry)
        a.D = D
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_UNSUPPORTED and ("outside [2,256]" if first else "outside [2,1024]") in msg, (D, rc, msg)


@pytest.mark.parametrize("entry", WITH_DIRECTION)
def test_every_entry_point_refuses_directions_that_are_not_unit_axis_steps(hip, entry):
    for r in ((0, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, -1)):
        a = _Args(hip, entry=entry)
        a.r = r
        rc, msg = a.call()
        assert rc == hip.MCCNN_E_INVALID and "axis-aligned unit step" in msg, (r, rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_point_refuses_short_flag_planes(hip, entry):
    a = _Args(hip, entry=entry)
    a.flags_bytes -= 1
    rc, msg = a.call()
    assert rc == hip.MCCNN_E_SCRATCH and "scratch" in msg, (rc, msg)


def test_abi_version_is_unchanged(hip):
    assert hip.load().mccnn_version() == 7 == hip.MCCNN_ABI_VERSION


# ---- the flag, the extra and the switch ------------------------------------------------------------------------------
def test_match_parser_accepts_paper_sgm_and_it_is_off_by_default():
    import match
    base = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]
    assert match.parser.parse_args(base).paper_sgm is False
    assert match.parser.parse_args(base + ["--paper_sgm"]).paper_sgm is True
    every = base + ["--paper_sgm", "--fast", "--separable_cbca", "--features", "library", "--pairs_in_flight", "2",
                    "--pipeline", "--readers", "2", "--arch", "accurate", "--num_fc_layers", "4", "--decision", "library",
                    "--paper_support_regions", "--paper_interpolation", "--numpy1_promotion", "--cbca_distance", "20"]
    args = match.parser.parse_args(every)
    assert args.paper_sgm and args.pipeline and args.fast and args.arch == "accurate"


class _StubNet(object):
    def supports_split_features(self):
        return True


def test_matcher_extra_defaults_off_and_unknown_extras_are_rejected(monkeypatch):
    import torch
    import stereo_device as sd
    monkeypatch.setattr(sd.hip, "require_device", lambda: torch.device("cpu"))
    m = sd.StereoMatcher(_StubNet())
    assert m.extras["sgm_independent_directions"] is False
    assert sd.StereoMatcher(_StubNet(), extras=dict(sgm_independent_directions=True)).extras["sgm_independent_directions"]
    # the extra changes neither the layout decision nor the workspace
    assert sd.StereoMatcher(_StubNet(), extras=dict(sgm_independent_directions=True)).pixel_major() == m.pixel_major()
    with pytest.raises(ValueError, match="unknown extras"):
        sd.StereoMatcher(_StubNet(), extras=dict(sgm_independent=True))
    with pytest.raises(ValueError, match="unknown extras"):
        sd.StereoMatcher(_StubNet(), extras=dict(no_such_option=True))


def test_module_switch_exists_and_is_off():
    import process_functional as pf
    assert pf.SGM_INDEPENDENT_DIRECTIONS is False
    import stereo_device as sd
    assert sd.SGM_ACC_MODES == (0, 1, 1, 2) and len(sd.SGM_DIRECTIONS) == 4
    assert tuple(sd.SGM_DIRECTIONS) == tuple(ps.DIRECTIONS)


# ---- why: accuracy on synthetic pairs --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,seed", [(96, 128, 32, 0), (96, 128, 32, 1), (128, 192, 48, 2)])
def test_paper_sgm_beats_the_sequential_composition_on_synthetic_pairs(net_layers, H, W, D, seed):
    """The whole pipeline on the CPU checker, trained weights, default hyper-parameters: the share of final pixels
    within 1 px of the true disparity is higher, and the mean absolute error lower, with the four independent directions
    averaged than with the reference's sequential composition.  The ordering is asserted, not the values."""
    import oracle as o
    import synthetic
    L, R, _, _, truth = synthetic.make_pair(H, W, D, seed=seed)
    fl, fr = o.net_features(L, net_layers), o.net_features(R, net_layers)
    cv = o.compute_cost_volume(fl, fr, D)
    truth = np.asarray(truth, np.float64).reshape(H, W)
    score = {}
    for independent in (False, True):
        out = ps.match_from_cost_volumes(L, R, cv[0], cv[1], D, independent).astype(np.float64)
        err = np.abs(out - truth)
        score[independent] = (float((err <= 1.0).mean()), float(err.mean()))
    print("%dx%dx%d seed %d: within 1 px %.3f -> %.3f, mean abs error %.2f -> %.2f px"
          % (H, W, D, seed, score[False][0], score[True][0], score[False][1], score[True][1]))
    assert score[True][0] > score[False][0], score
    assert score[True][1] < score[False][1], score
