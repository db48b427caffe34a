"""CPU: a pair's row offset (include/mccnn.h: mccnn_vertical_profile, mccnn_vertical_offset_select,
mccnn_cost_volume_offset_hwd) - the NumPy restatement tied to tests/vertical_reference.py and to the oracle, the
measurement on pairs that are 0 to 3 rows off, the validation of the entry points, the flags / extras / switch, and the
reason for it: matching along the measured offset recovers what the plain matcher loses on such a pair."""
import ctypes

import numpy as np
import pytest

from helpers import assert_bits
import paper_sgm_reference as ps
import vertical_offset_reference as vo
import vertical_reference as vr

PAIRS = [(96, 128, 32, 0), (96, 128, 32, 1), (128, 192, 48, 2)]
README_RANGE_2 = {0: 0.747, 1: 0.687, 2: 0.683}     # the README's column: two rows off, vertical_range=2, by seed


def _random_features(H, W, seed):
    rng = np.random.RandomState(seed)
    return tuple(rng.standard_normal((H, W, 64)).astype(np.float32) for _ in range(2))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,seed", [(3, 37, 11, 0), (6, 23, 21, 1)])
def test_offset_0_equals_the_vertical_restatement(H, W, D, seed):
    fl, fr = _random_features(H, W, seed)
    for r in (0, 1, 2):
        want = vr.compute_cost_volume_vertical(fl, fr, D, r)
        got = vo.compute_cost_volume_offset(fl, fr, D, 0, r)
        assert_bits(got[0], want[0], "range %d, left" % r)
        assert_bits(got[1], want[1], "range %d, right" % r)


@pytest.mark.parametrize("dy", [-3, -1, 2])
def test_offset_equals_the_oracle_on_moved_features_where_no_row_is_clamped(dy):
    """The right features moved dy rows down, matched along offset dy: the plain volumes of the pair that was not moved,
    on the rows whose partner row h + dy (left view) or h - dy (right view) exists."""
    import oracle as o
    H, W, D = 9, 40, 12
    fl, fr = _random_features(H, W, 5)
    want = o.compute_cost_volume(fl, fr, D)
    got = vo.compute_cost_volume_offset(fl, vr.shift_rows(fr, dy), D, dy, 0)
    rows_l = slice(max(0, -dy), min(H, H - dy))                # left row h against moved row h + dy = right row h
    assert_bits(got[0][:, rows_l], want[0][:, rows_l], "left")
    # right volume row h' of the moved image is right row h' - dy of the pair
    rows_r = slice(max(0, dy), min(H, H + dy))
    moved_back = slice(rows_r.start - dy, rows_r.stop - dy)
    assert_bits(got[1][:, rows_r], want[1][:, moved_back], "right")
    assert not np.array_equal(vo.compute_cost_volume_offset(fl, vr.shift_rows(fr, dy), D, 0, 0)[0][:, rows_l],
                              want[0][:, rows_l])


def test_offset_follows_the_definition_pixel_by_pixel():
    """A scalar loop over the definition on a tiny shape: both views, the clamped rows, the stored value clamped to +-8."""
    H, W, D = 5, 9, 3
    fl, fr = _random_features(H, W, 3)

    def p(hl, wl, hr, wr):
        return np.sum(fl[hl, wl] * fr[hr, wr], dtype=np.float32)

    for k0, r in ((2, 1), (-3, 0), (8, 1), (-6, 4)):
        sl, sr = vo.offset_scores(fl, fr, D, k0, r)
        for d in range(D):
            for h in range(H):
                ks = [k for k in range(k0 - r, k0 + r + 1) if 0 <= h + k < H] or [min(max(k0, -h), H - 1 - h)]
                for w in range(d, W):
                    assert sl[d, h, w] == max(p(h, w, h + k, w - d) for k in ks)
                ks = [k for k in range(k0 - r, k0 + r + 1) if 0 <= h - k < H] or [min(max(k0, h - (H - 1)), h)]
                for w in range(W - d):
                    assert sr[d, h, w] == max(p(h - k, w + d, h, w) for k in ks)
    a, b = vo.compute_cost_volume_offset(fl, fr, D, 2 ** 31 - 1, 1), vo.compute_cost_volume_offset(fl, fr, D, 8, 1)
    assert_bits(a[0], b[0], "a stored 2^31 - 1 is 8")


def test_profile_follows_the_definition_pixel_by_pixel():
    H, W, D, R, step = 7, 70, 5, 2, 3
    fl, fr = _random_features(H, W, 4)
    fl[4, 10, 3] = np.float32("nan")
    votes = vo.vertical_profile(fl, fr, D, R, step)
    assert votes.shape == (2, 2, 5) and votes.dtype == np.uint32 and vo.profile_rows(H, step) == 2
    want = np.zeros_like(votes)
    for i, h in enumerate((1, 4)):
        for w in range(W):
            b = {}
            for k in range(-R, R + 1):
                if 0 <= h + k < H:
                    b[k] = [np.sum(fl[h, w] * fr[h + k, w - d], dtype=np.float32) for d in range(min(D - 1, w) + 1)]
            if any(np.isnan(v).any() for v in b.values()):
                continue
            best, winner = max(b[0]), 0
            for k in (-1, 1, -2, 2):
                if k in b and max(b[k]) > best:
                    best, winner = max(b[k]), k
            want[i, w // 64, winner + R] += 1
    assert np.array_equal(votes, want)
    assert int(votes[1].sum()) == W - 1 and int(votes[0].sum()) == W
    assert [vo.profile_rows(H, s) for H, s in ((7, 1), (7, 8), (7, 14), (7, 16), (1, 1), (40, 8))] == [7, 1, 0, 0, 1, 5]


def test_select_breaks_ties_towards_the_smaller_offset_and_no_votes_give_0():
    assert vo.candidate_order(3) == [0, -1, 1, -2, 2, -3, 3]
    votes = np.zeros((2, 1, 5), np.uint32)
    assert vo.offset_select(votes, 2)[0] == 0
    votes[0, 0] = [4, 7, 0, 7, 4]
    assert vo.offset_select(votes, 2)[0] == -1                   # -1 comes before +1
    votes[1, 0] = [4, 0, 7, 0, 4]
    offset, totals = vo.offset_select(votes, 2)
    assert offset == -2 and list(totals) == [8, 7, 7, 7, 8] and totals.dtype == np.uint64   # +-2 lead with 8 each: -2 first
    votes[1, 0, 4] += 1
    assert vo.offset_select(votes, 2)[0] == 2
    assert vo.share(np.array([1, 0, 3], np.uint64), 1, 1) == 0.75 and vo.share(np.zeros(3, np.uint64), 0, 1) == 0.0
    flat = np.zeros((4, 70, 64), np.float32)
    assert int(vo.vertical_profile(flat, flat, 8, 2, 1)[:, :, 2].sum()) == 4 * 70      # a flat image votes 0


# ---- the measurement and the accuracy on pairs that are off ----------------------------------------------------------------
_PAIR = {}


def _pair(net_layers, H, W, D, seed):
    """The synthetic pair, its truth and a cache of the right view's features by dy (computed once, never changed)."""
    import oracle as o
    import synthetic
    key = (H, W, D, seed)
    if key not in _PAIR:
        L, R, _, _, truth = synthetic.make_pair(H, W, D, seed=seed)
        _PAIR[key] = dict(L=L, R=R, truth=np.asarray(truth, np.float64).reshape(H, W), fl=o.net_features(L, net_layers),
                          moved={}, fr={})
    c = _PAIR[key]

    def right(dy):
        if dy not in c["fr"]:
            c["moved"][dy] = vr.shift_rows(c["R"], dy)
            c["fr"][dy] = o.net_features(c["moved"][dy], net_layers)
        return c["moved"][dy], c["fr"][dy]
    return c, right


@pytest.mark.parametrize("H,W,D,seed", PAIRS)
def test_profile_and_select_measure_the_offset(net_layers, H, W, D, seed):
    c, right = _pair(net_layers, H, W, D, seed)
    for dy in (-3, 0, 1, 2):
        _, fr = right(dy)
        votes = vo.vertical_profile(c["fl"], fr, D, 4, 4)
        offset, totals = vo.offset_select(votes, 4)
        print("%dx%dx%d seed %d, dy %+d: offset %+d, share %.3f, totals %s"
              % (H, W, D, seed, dy, offset, vo.share(totals, offset, 4), [int(t) for t in totals]))
        assert offset == dy, (dy, offset, totals)


@pytest.mark.parametrize("H,W,D,seed", PAIRS)
def test_matching_along_the_offset_recovers_a_pair_that_is_two_rows_off(net_layers, H, W, D, seed):
    """The whole pipeline on the CPU checker, trained weights, default hyper-parameters, the paper's SGM: the share of
    final pixels within 1 px of the truth (four top and bottom rows left out).  Two rows off, the run along offset 2
    exceeds the plain run by more than 0.10 (measured gaps 0.13 to 0.21) and lies within 0.03 of the aligned pair
    (measured 0.004 to 0.019)."""
    import oracle as o
    c, right = _pair(net_layers, H, W, D, seed)

    def share(image, cv):
        return vr.within_1px(ps.match_from_cost_volumes(c["L"], image, cv[0], cv[1], D, True), c["truth"])

    aligned = share(c["R"], o.compute_cost_volume(c["fl"], right(0)[1], D))
    moved, fr = right(2)
    plain = share(moved, o.compute_cost_volume(c["fl"], fr, D))
    along = share(moved, vo.compute_cost_volume_offset(c["fl"], fr, D, 2, 0))
    print("%dx%dx%d seed %d: aligned %.3f; two rows off: plain %.3f, vertical_range=2 %.3f (README), offset 2 %.3f"
          % (H, W, D, seed, aligned, plain, README_RANGE_2[seed], along))
    assert along - plain > 0.10, (aligned, plain, along)
    assert abs(aligned - along) <= 0.03, (aligned, plain, along)


# ---- the entry points: validation before any launch --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import _hipabi
    _hipabi.load()
    return _hipabi


FL, FR, LCV, RCV, K0, VOTES, TOTALS = (ctypes.c_void_p(a) for a in (0x10000000, 0x20000000, 0x30000000, 0x40000000,
                                                                    0x50000000, 0x60000000, 0x70000000))


def _offset(hip, H=4, W=12, C=64, D=8, r=2, fl=FL, fr=FR, lcv=LCV, rcv=RCV, k0=K0):
    lib = hip.load()
    rc = lib.mccnn_cost_volume_offset_hwd(fl, fr, H, W, C, D, k0, r, lcv, rcv, None)
    return rc, lib.mccnn_last_error_string().decode()


def _profile(hip, H=4, W=12, C=64, D=8, R=2, step=1, nbytes=None, fl=FL, fr=FR, votes=VOTES):
    lib = hip.load()
    if nbytes is None:
        nbytes = 4 * lib.mccnn_vertical_profile_rows(H, max(step, 1)) * ((W + 63) // 64) * (2 * abs(R) + 1)
    rc = lib.mccnn_vertical_profile(fl, fr, H, W, C, D, R, step, votes, nbytes, None)
    return rc, lib.mccnn_last_error_string().decode()


def _select(hip, rows=2, blocks=1, R=2, votes=VOTES, offset=K0, totals=TOTALS):
    lib = hip.load()
    rc = lib.mccnn_vertical_offset_select(votes, rows, blocks, R, offset, totals, None)
    return rc, lib.mccnn_last_error_string().decode()


def test_entries_refuse_null_pointers(hip):
    for name in ("fl", "fr", "lcv", "rcv"):
        for k0 in (K0, None):                                 # (a null offset means 0, it is no error)
            rc, msg = _offset(hip, k0=k0, **{name: None})
            assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg, (name, rc, msg)
    for name in ("fl", "fr", "votes"):
        rc, msg = _profile(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg, (name, rc, msg)
    for name in ("votes", "offset", "totals"):
        rc, msg = _select(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg, (name, rc, msg)


def test_entries_refuse_ranges_and_offsets_outside_their_limits(hip):
    for r in (-1, 5):
        rc, msg = _offset(hip, r=r)
        assert rc == hip.MCCNN_E_INVALID and "vertical_range=%d" % r in msg and "[0, 4]" in msg, (rc, msg)
    for R in (-1, 9):
        rc, msg = _profile(hip, R=R)
        assert rc == hip.MCCNN_E_INVALID and "max_offset=%d" % R in msg and "[0, 8]" in msg, (rc, msg)
        rc, msg = _select(hip, R=R)
        assert rc == hip.MCCNN_E_INVALID and "max_offset=%d" % R in msg and "[0, 8]" in msg, (rc, msg)
    for step in (0, -2):
        rc, msg = _profile(hip, step=step)
        assert rc == hip.MCCNN_E_INVALID and "row_step=%d" % step in msg, (rc, msg)
    rc, msg = _select(hip, rows=-1)
    assert rc == hip.MCCNN_E_INVALID, (rc, msg)


def test_profile_refuses_a_short_votes_buffer(hip):
    need = 4 * 4 * 1 * 5
    rc, msg = _profile(hip, nbytes=need - 1)
    assert rc == hip.MCCNN_E_SCRATCH and "%d bytes" % need in msg, (rc, msg)
    assert hip.load().mccnn_vertical_profile_rows(40, 8) == 5 and hip.load().mccnn_vertical_profile_rows(7, 14) == 0
    assert hip.load().mccnn_vertical_profile_rows(7, 0) == 0


@pytest.mark.parametrize("call", [_offset, _profile])
def test_entries_keep_the_envelope_of_the_vertical_search(hip, call):
    for D in (0, 1, 1025):
        rc, msg = call(hip, W=2000, D=D)
        assert rc == hip.MCCNN_E_UNSUPPORTED and "D=%d" % D in msg and "[2, 1024]" in msg, (rc, msg)
    rc, msg = call(hip, W=12, D=11)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "W >= D+2" in msg, (rc, msg)
    rc, msg = call(hip, C=112)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "64 channels" in msg, (rc, msg)
    rc, msg = call(hip, H=0)
    assert rc == hip.MCCNN_E_INVALID and "non-positive" in msg, (rc, msg)
    rc, msg = call(hip, H=65536)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "65535" in msg, (rc, msg)


def test_abi_version_is_unchanged_and_the_symbols_are_in_the_table(hip):
    assert hip.load().mccnn_version() == 7 == hip.MCCNN_ABI_VERSION
    for name in ("mccnn_vertical_profile_rows", "mccnn_vertical_profile", "mccnn_vertical_offset_select",
                 "mccnn_cost_volume_offset_hwd"):
        assert name in hip.SIGNATURES


# ---- the flags, the extras and the switch ----------------------------------------------------------------------------------
BASE = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]


def test_match_parser_accepts_the_flags_and_their_defaults_ask_for_nothing():
    import match
    args = match.parser.parse_args(BASE)
    assert (args.vertical_offset, args.vertical_offset_max, args.vertical_offset_rows) == ("0", 4, 8)
    assert match.parse_vertical_offset(args.vertical_offset) == 0
    assert match.parse_vertical_offset("auto") == "auto" and match.parse_vertical_offset("-8") == -8
    assert [match.parse_vertical_offset(t) for t in ("9", "-9", "1.5", "Auto", "")] == [None] * 5
    every = BASE + ["--vertical_offset", "auto", "--vertical_offset_max", "8", "--vertical_offset_rows", "4",
                    "--vertical_range", "1", "--views", "both", "--confidence", "msm", "--evaluate", "--paper_sgm",
                    "--pairs_in_flight", "2", "--pipeline", "--dataset", "kitti2015"]
    args = match.parser.parse_args(every)
    assert (args.vertical_offset, args.vertical_offset_max, args.vertical_offset_rows) == ("auto", 8, 4)
    assert match.parser.parse_args(BASE + ["--vertical_offset", "-3"]).vertical_offset == "-3"


@pytest.mark.parametrize("value", ["auto", "2"])
@pytest.mark.parametrize("extra,reason", [(["--fast"], "--fast"), (["--fast", "--separable_cbca"], "--fast"),
                                          (["--separable_cbca"], "--separable_cbca"),
                                          (["--arch", "accurate"], "--arch accurate"),
                                          (["--paper_support_regions"], "--paper_support_regions")])
def test_match_refuses_the_offset_where_it_refuses_the_vertical_range(value, extra, reason, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + ["--vertical_offset", value] + extra)
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert "--vertical_offset is not available with %s" % reason in err, err


@pytest.mark.parametrize("flags,text", [(["--vertical_offset", "9"], "neither 'auto' nor an integer in [-8, 8]"),
                                        (["--vertical_offset", "up"], "neither 'auto' nor an integer in [-8, 8]"),
                                        (["--vertical_offset_max", "0"], "outside [1, 8]"),
                                        (["--vertical_offset_max", "9"], "outside [1, 8]"),
                                        (["--vertical_offset_rows", "0"], "< 1")])
def test_match_refuses_values_outside_the_limits(flags, text, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + flags)
    assert e.value.code != 0 and text in capsys.readouterr().err


def test_layouts_name_the_file_of_the_measurement():
    import datasets
    want = {"middlebury": "/out/submit_t/trainingH/pairA/verticalMCCNN.json", "kitti2015": "/out/submit_t/vertical/000007_10.json",
            "kitti2012": "/out/submit_t/vertical/000007_10.json"}
    for name in datasets.NAMES:
        layout = datasets.get(name)
        left = "/data/training/image_2/000007_10.png" if layout.kitti else "/data/trainingH/pairA/im0.png"
        paths = layout.outputs(left, "/data", "/out/submit_t", "/out/submit_t_imgs")
        assert layout.vertical_path(paths) == want[name]


class _StubNet(object):
    def supports_split_features(self):
        return True


class _StubAccurateNet(object):
    fc_weights = ()

    def supports_split_features(self):
        return False


@pytest.fixture
def sd(monkeypatch):
    import torch
    import stereo_device
    monkeypatch.setattr(stereo_device.hip, "require_device", lambda: torch.device("cpu"))
    return stereo_device


def test_matcher_extras_default_to_nothing_and_change_no_route(sd):
    m = sd.StereoMatcher(_StubNet())
    assert (m.extras["vertical_offset"], m.extras["vertical_offset_max"], m.extras["vertical_offset_rows"]) == (0, 4, 8)
    for value in (2, -8, "auto"):
        v = sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset=value))
        assert v.extras["vertical_offset"] == value
        assert v.pixel_major() == m.pixel_major() and v.route(40, 48, 16) == m.route(40, 48, 16)
    kernel = m.workspace_cbca_kernel(40, 96, 24)
    base = sd.workspace_bytes(40, 96, 24, True, kernel)
    assert sd.workspace_bytes(40, 96, 24, True, kernel, vertical_offset=0, vertical_offset_max=8) == base
    assert sd.workspace_bytes(40, 96, 24, True, kernel, vertical_offset=3) == base + 4 + 8 * 9 + 4 * 5 * 2 * 9
    assert sd.workspace_bytes(40, 96, 24, True, kernel, vertical_offset="auto", vertical_offset_max=8, vertical_offset_rows=1,
                              pairs_in_flight=2) == 2 * (base + 4 + 8 * 17 + 4 * 40 * 2 * 17)
    # with everything downstream that the default route offers
    sd.StereoMatcher(_StubNet(), hp=dict(cbca_distance=32), confidence=("msm",), views="both", semi_dense="lr",
                     extras=dict(vertical_offset="auto", vertical_offset_max=8, vertical_offset_rows=1, vertical_range=4,
                                 sgm_independent_directions=True))
    with pytest.raises(ValueError, match="unknown extras"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_offsets=2))


@pytest.mark.parametrize("extras,text", [(dict(vertical_offset=9), r"vertical_offset must be 'auto' or an integer in \[-8, 8\]"),
                                         (dict(vertical_offset=-9), "vertical_offset must be"),
                                         (dict(vertical_offset=1.0), "vertical_offset must be"),
                                         (dict(vertical_offset=True), "vertical_offset must be"),
                                         (dict(vertical_offset="2"), "vertical_offset must be"),
                                         (dict(vertical_offset_max=0), r"vertical_offset_max must be an integer in \[1, 8\]"),
                                         (dict(vertical_offset_max=9), "vertical_offset_max must be"),
                                         (dict(vertical_offset_rows=0), "vertical_offset_rows must be an integer >= 1"),
                                         (dict(vertical_offset_rows=2.0), "vertical_offset_rows must be")])
def test_matcher_refuses_values_outside_the_limits(sd, extras, text):
    with pytest.raises(ValueError, match=text):
        sd.StereoMatcher(_StubNet(), extras=extras)


@pytest.mark.parametrize("value", [1, "auto"])
def test_matcher_refuses_the_configurations_without_a_vertical_search(sd, value):
    ex = dict(vertical_offset=value)
    with pytest.raises(ValueError, match="vertical_offset=.*accurate network"):
        sd.StereoMatcher(_StubAccurateNet(), extras=ex)
    with pytest.raises(ValueError, match="vertical_offset=.*MCCNN_CV_MFMA"):
        sd.StereoMatcher(_StubNet(), cv_mode=sd.hip.MCCNN_CV_MFMA, extras=ex)
    with pytest.raises(ValueError, match="vertical_offset=.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), layout="plane_major", extras=ex)
    with pytest.raises(ValueError, match="vertical_offset=.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), cbca_order=sd.hip.MCCNN_CBCA_SEPARABLE, extras=ex)
    with pytest.raises(ValueError, match="vertical_offset=.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset=value, both_view_support=True))
    # offset 0 asks for nothing: all of them stand
    sd.StereoMatcher(_StubAccurateNet(), extras=dict(vertical_offset=0))
    sd.StereoMatcher(_StubNet(), cv_mode=sd.hip.MCCNN_CV_MFMA, layout="plane_major", extras=dict(vertical_offset=0))
    # the vertical range's own refusals keep their words
    with pytest.raises(ValueError, match="vertical_range=1: the accurate network's decision stage has no vertical search"):
        sd.StereoMatcher(_StubAccurateNet(), extras=dict(vertical_range=1, vertical_offset=value))


def test_module_switch_exists_and_is_0():
    import process_functional as pf
    import stereo_device
    assert pf.VERTICAL_OFFSET == 0 and "vertical_profile" in pf.__all__
    assert stereo_device.VERTICAL_OFFSET_MAX == 8
    assert stereo_device.vertical_record(np.array([2], np.int32), np.array([1, 0, 0, 0, 6, 0, 1], np.int64)) == \
        dict(offset=2, totals=[1, 0, 0, 0, 6, 0, 1], share=0.0)                 # max 3: offset 2 is index 5
    assert stereo_device.vertical_record([1], [1, 0, 3]) == dict(offset=1, totals=[1, 0, 3], share=0.75)


# ---- with the defaults none of the new calls is made -------------------------------------------------------------------
class _Recorder(object):
    """Stands in front of the loaded library: records the cost-volume and measurement calls and refuses them (nothing
    may reach a device from this test); the host-side queries (mccnn_hwd_pitch, ...) pass."""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        if name not in NEW_CALLS + ("mccnn_cost_volume", "mccnn_cost_volume_hwd", "mccnn_cost_volume_vertical_hwd"):
            return getattr(self._lib, name)

        def call(*args):
            self.called.append(name)
            raise _Called(name)
        return call


class _Called(Exception):
    pass


NEW_CALLS = ("mccnn_vertical_profile", "mccnn_vertical_offset_select", "mccnn_cost_volume_offset_hwd")


def test_defaults_reach_none_of_the_new_entry_points(sd, monkeypatch):
    import torch
    rec = _Recorder(sd.hip.load())
    monkeypatch.setattr(sd.hip, "load", lambda: rec)
    monkeypatch.setattr(sd.hip, "ptr", lambda t: None)
    monkeypatch.setattr(sd.hip, "stream", lambda: None)
    fl = fr = torch.zeros((4, 12, 64))
    hwd = [torch.zeros((4, 12, 8)) for _ in range(4)]

    class _Timer(object):
        def start(self, name):
            pass

        def stop(self):
            pass

    def first_call(extras, ws):
        del rec.called[:]
        m = sd.StereoMatcher(_StubNet(), extras=extras)
        with pytest.raises(_Called):
            m._cost_volumes(fl, fr, 8, hwd, hwd, _Timer(), ws)
        return rec.called[0]

    assert first_call({}, None) == "mccnn_cost_volume_hwd"
    assert first_call(dict(vertical_offset=0, vertical_offset_max=8, vertical_offset_rows=1), None) == "mccnn_cost_volume_hwd"
    assert first_call(dict(vertical_range=2), None) == "mccnn_cost_volume_vertical_hwd"
    ws = dict(v_offset=torch.zeros(1, dtype=torch.int32), v_totals=torch.zeros(9, dtype=torch.int64),
              v_votes=torch.zeros((1, 1, 9), dtype=torch.int32))
    assert first_call(dict(vertical_offset=2), ws) == "mccnn_cost_volume_offset_hwd"
    monkeypatch.setattr(sd, "vertical_profile_shape", lambda H, W, R, step: (1, 1, 2 * R + 1))
    assert first_call(dict(vertical_offset="auto"), ws) == "mccnn_vertical_profile"
    assert set(NEW_CALLS) <= set(sd.hip.SIGNATURES)
