"""CPU: a field of row offsets (include/mccnn.h: mccnn_vertical_field_select, mccnn_cost_volume_field_hwd) - the NumPy
restatement tied to tests/vertical_offset_reference.py, the selection per cell, the validation of the entry points, the
flags / extras / switch, and the reason for it: on a pair sheared by whole rows, whose mean offset is zero, matching along
the measured field recovers what the plain matcher and the single measured offset lose."""
import ctypes

import numpy as np
import pytest

from helpers import assert_bits
import paper_sgm_reference as ps
import vertical_field_reference as vf
import vertical_offset_reference as vo
import vertical_reference as vr


def _random_features(H, W, seed):
    rng = np.random.RandomState(seed)
    return tuple(rng.standard_normal((H, W, 64)).astype(np.float32) for _ in range(2))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,grid", [(5, 70, 9, (2, 2)), (7, 130, 21, (3, 3))])
def test_constant_field_equals_the_offset_restatement(H, W, D, grid):
    fl, fr = _random_features(H, W, H)
    for k in (-8, -3, 0, 2, 8):
        for r in (0, 1):
            want = vo.compute_cost_volume_offset(fl, fr, D, k, r)
            for g in (grid, (1, 1)):
                got = vf.compute_cost_volume_field(fl, fr, D, np.full(g, k, np.int32), r)
                assert_bits(got[0], want[0], "k %d, range %d, grid %s, left" % (k, r, g))
                assert_bits(got[1], want[1], "k %d, range %d, grid %s, right" % (k, r, g))


def test_field_follows_the_definition_pixel_by_pixel():
    """A scalar loop over the definition: a 3 x 3 field of mixed signs on 6 x 130 x 5, both views; the right view takes
    the cell of its partner's column w + d, which for w = 60 .. 63 and 124 .. 127 lies in another band than w."""
    H, W, D = 6, 130, 5
    fl, fr = _random_features(H, W, 3)
    field = np.array([[2, -1, 0], [-3, 1, 4], [0, -2, 3]], np.int32)
    rb, cb = vf.row_bands(H, 3), vf.column_bands(W, 3)
    assert list(rb) == [0, 0, 1, 1, 2, 2] and [int(cb[x]) for x in (0, 63, 64, 127, 128, 129)] == [0, 0, 1, 1, 2, 2]

    def p(hl, wl, hr, wr):
        return np.sum(fl[hl, wl] * fr[hr, wr], dtype=np.float32)

    crossed = 0
    for r in (0, 1):
        sl, sr = vf.field_scores(fl, fr, D, field, r)
        for d in range(D):
            for h in range(H):
                for w in range(d, W):
                    k0 = int(field[rb[h], cb[w]])
                    ks = [k for k in range(k0 - r, k0 + r + 1) if 0 <= h + k < H] or [min(max(k0, -h), H - 1 - h)]
                    assert sl[d, h, w] == max(p(h, w, h + k, w - d) for k in ks)
                for w in range(W - d):
                    k0 = int(field[rb[h], cb[w + d]])
                    crossed += cb[w + d] != cb[w]
                    ks = [k for k in range(k0 - r, k0 + r + 1) if 0 <= h - k < H] or [min(max(k0, h - (H - 1)), h)]
                    assert sr[d, h, w] == max(p(h - k, w + d, h, w) for k in ks)
    assert crossed > 0
    wild = np.array([[1000, -2 ** 31]], np.int64)
    a, b = vf.compute_cost_volume_field(fl, fr, D, wild, 1), vf.compute_cost_volume_field(fl, fr, D, [[8, -8]], 1)
    assert_bits(a[0], b[0], "stored 1000 and INT32_MIN are 8 and -8")
    assert_bits(a[1], b[1], "stored 1000 and INT32_MIN are 8 and -8, right")


# ---- the selection -----------------------------------------------------------------------------------------------------
def test_a_1x1_grid_selects_what_offset_select_selects():
    rng = np.random.RandomState(0)
    votes = rng.randint(0, 50, size=(5, 3, 9)).astype(np.uint32)
    field, totals, offset, global_totals = vf.field_select(votes, 40, 8, 4, 1, 1)
    want, want_totals = vo.offset_select(votes, 4)
    assert field.shape == (1, 1) and field.dtype == np.int32 and int(field[0, 0]) == want == offset
    assert np.array_equal(totals[0, 0], want_totals) and np.array_equal(global_totals, want_totals)
    assert totals.dtype == np.uint64


def test_select_per_cell_ties_and_cells_without_votes():
    # H = 10, row_step 2: profiled rows 1 3 5 7 9; gh = 3: bands of rows 0..3 | 4..6 | 7..9 -> rows (1 3) (5) (7 9)
    H, step, R = 10, 2, 2
    votes = np.zeros((5, 3, 5), np.uint32)
    votes[0, 0] = [0, 3, 1, 0, 0]         # cell (0, 0): -1 leads
    votes[1, 0] = [0, 0, 1, 0, 2]         #              ... 3 for -1, 2 for 0, 2 for +2
    votes[2, 1] = [4, 0, 0, 0, 4]         # cell (1, 1): -2 and +2 tie: the negative one
    votes[3, 2] = [0, 5, 0, 5, 0]         # cell (2, 2): -1 and +1 tie ...
    votes[4, 2] = [6, 0, 0, 0, 0]         #              ... and -2 beats both
    votes[4, 0] = [0, 2, 2, 2, 0]         # cell (2, 0): 0, -1, +1 tie: the smaller |k|
    field, totals, offset, global_totals = vf.field_select(votes, H, step, R, 3, 3)
    assert list(global_totals) == [10, 10, 4, 7, 6] and offset == -1       # -1 before -2 at 10 each
    assert field.tolist() == [[-1, -1, -1], [-1, -2, -1], [0, -1, -2]]       # cells without a vote: the global -1
    assert totals[0, 0].tolist() == [0, 3, 2, 0, 2] and totals[2, 2].tolist() == [6, 5, 0, 5, 0]
    assert int(totals.sum()) == int(votes.sum())
    none = vf.field_select(np.zeros((5, 3, 5), np.uint32), H, step, R, 2, 3)
    assert not none[0].any() and none[2] == 0


def test_grid_mapping_at_block_and_band_edges():
    assert vf.column_bands(64, 1).tolist() == [0] * 64
    assert vf.column_bands(65, 2).tolist() == [0] * 64 + [1]
    c = vf.column_bands(129, 2)                      # three blocks on two bands: 0 0 1
    assert c[63] == 0 and c[64] == 0 and c[127] == 0 and c[128] == 1
    c = vf.column_bands(129, 3)
    assert c[63] == 0 and c[64] == 1 and c[128] == 2
    assert vf.column_bands(500, 4).tolist() == sum(([b] * n for b, n in ((0, 128), (1, 128), (2, 128), (3, 116))), [])
    assert vf.row_bands(7, 3).tolist() == [0, 0, 0, 1, 1, 2, 2]             # 7 is no multiple of 3
    assert vf.row_bands(10, 4).tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]
    # a cell without a profiled row: H = 7, step 4 profiles rows 2 and 6; bands 0 0 0 1 1 2 2 -> band 1 has none
    votes = np.zeros((2, 1, 3), np.uint32)
    votes[0, 0, 2], votes[1, 0, 0] = 3, 2
    field, totals, offset, _ = vf.field_select(votes, 7, 4, 1, 3, 1)
    assert offset == 1 and field.tolist() == [[1], [1], [-1]] and not totals[1].any()


# ---- the entry points: validation before any launch --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import _hipabi
    _hipabi.load()
    return _hipabi


FL, FR, LCV, RCV, FIELD, VOTES, TOTALS, OFFSET, GLOBAL = (ctypes.c_void_p(a << 28) for a in range(1, 10))


def _volume(hip, H=4, W=130, C=64, D=8, gh=2, gw=3, r=1, fl=FL, fr=FR, field=FIELD, lcv=LCV, rcv=RCV):
    lib = hip.load()
    rc = lib.mccnn_cost_volume_field_hwd(fl, fr, H, W, C, D, field, gh, gw, r, lcv, rcv, None)
    return rc, lib.mccnn_last_error_string().decode()


def _select(hip, rows=5, blocks=3, H=40, step=8, R=2, gh=2, gw=3, votes=VOTES, field=FIELD, totals=TOTALS, offset=OFFSET,
            global_totals=GLOBAL):
    lib = hip.load()
    rc = lib.mccnn_vertical_field_select(votes, rows, blocks, H, step, R, gh, gw, field, totals, offset, global_totals, None)
    return rc, lib.mccnn_last_error_string().decode()


def test_entries_refuse_null_pointers(hip):
    for name in ("fl", "fr", "field", "lcv", "rcv"):
        rc, msg = _volume(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "mccnn_cost_volume_field_hwd: null pointer" in msg, (name, rc, msg)
    for name in ("votes", "field", "totals", "offset", "global_totals"):
        rc, msg = _select(hip, **{name: None})
        assert rc == hip.MCCNN_E_INVALID and "mccnn_vertical_field_select: null pointer" in msg, (name, rc, msg)


@pytest.mark.parametrize("call", [_volume, _select])
def test_entries_refuse_a_grid_outside_its_limits_and_name_the_argument(hip, call):
    for name in ("gh", "gw"):
        for value in (0, -1, 9):
            rc, msg = call(hip, **{name: value})
            assert rc == hip.MCCNN_E_INVALID and "%s=%d" % (name, value) in msg and "[1, 8]" in msg, (rc, msg)
    rc, msg = call(hip, gw=4)                         # 130 columns, or 3 blocks
    assert rc == hip.MCCNN_E_INVALID and "gw=4" in msg and "3" in msg, (rc, msg)
    rc, msg = call(hip, **(dict(H=4, gh=5) if call is _volume else dict(H=4, step=1, rows=4, gh=5)))
    assert rc == hip.MCCNN_E_INVALID and "gh=5" in msg and "H=4" in msg, (rc, msg)


def test_entries_refuse_the_other_arguments_as_the_offset_calls_do(hip):
    for r in (-1, 5):
        rc, msg = _volume(hip, r=r)
        assert rc == hip.MCCNN_E_INVALID and "vertical_range=%d" % r in msg and "[0, 4]" in msg, (rc, msg)
    for D in (0, 1, 1025):
        rc, msg = _volume(hip, W=2000, D=D)
        assert rc == hip.MCCNN_E_UNSUPPORTED and "D=%d" % D in msg and "[2, 1024]" in msg, (rc, msg)
    rc, msg = _volume(hip, W=130, D=129)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "W >= D+2" in msg, (rc, msg)
    rc, msg = _volume(hip, C=112)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "64 channels" in msg, (rc, msg)
    rc, msg = _volume(hip, H=0)
    assert rc == hip.MCCNN_E_INVALID and "non-positive" in msg, (rc, msg)
    rc, msg = _volume(hip, H=65536)
    assert rc == hip.MCCNN_E_UNSUPPORTED and "65535" in msg, (rc, msg)
    for R in (-1, 9):
        rc, msg = _select(hip, R=R)
        assert rc == hip.MCCNN_E_INVALID and "max_offset=%d" % R in msg and "[0, 8]" in msg, (rc, msg)
    rc, msg = _select(hip, step=0)
    assert rc == hip.MCCNN_E_INVALID and "row_step=0" in msg, (rc, msg)
    rc, msg = _select(hip, H=0)
    assert rc == hip.MCCNN_E_INVALID and "H=0" in msg, (rc, msg)
    rc, msg = _select(hip, rows=4)                    # 40 rows at step 8 profile 5
    assert rc == hip.MCCNN_E_INVALID and "n_rows=4" in msg and "5" in msg, (rc, msg)
    rc, msg = _select(hip, blocks=0, gw=1)
    assert rc == hip.MCCNN_E_INVALID and "n_blocks=0" in msg, (rc, msg)


def test_abi_version_is_unchanged_and_the_symbols_are_in_the_table(hip):
    assert hip.load().mccnn_version() == 7 == hip.MCCNN_ABI_VERSION
    for name in ("mccnn_vertical_field_select", "mccnn_cost_volume_field_hwd"):
        assert name in hip.SIGNATURES and hasattr(hip.load(), name)
    assert len(hip.SIGNATURES["mccnn_vertical_field_select"][1]) == 13
    assert len(hip.SIGNATURES["mccnn_cost_volume_field_hwd"][1]) == 13


# ---- the flags, the extras and the switch ----------------------------------------------------------------------------------
BASE = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]


def test_match_parser_accepts_the_flags_and_their_defaults_ask_for_nothing():
    import match
    args = match.parser.parse_args(BASE)
    assert (args.vertical_offset, args.vertical_offset_grid) == ("0", "3x4")
    assert match.parse_vertical_offset("grid") == "grid" and match.parse_vertical_offset("auto") == "auto"
    assert match.parse_vertical_offset("Grid") is None and match.parse_vertical_offset("3") == 3
    assert match.parse_vertical_offset_grid("3x4") == (3, 4) and match.parse_vertical_offset_grid("8X1") == (8, 1)
    assert [match.parse_vertical_offset_grid(t) for t in ("0x4", "3x9", "3", "3x4x5", "axb", "", "3x")] == [None] * 7
    every = BASE + ["--vertical_offset", "grid", "--vertical_offset_grid", "2x5", "--vertical_offset_max", "8",
                    "--vertical_offset_rows", "4", "--vertical_range", "1", "--views", "both", "--confidence", "msm",
                    "--evaluate", "--paper_sgm", "--pairs_in_flight", "2", "--pipeline", "--dataset", "kitti2015"]
    args = match.parser.parse_args(every)
    assert (args.vertical_offset, args.vertical_offset_grid) == ("grid", "2x5")


@pytest.mark.parametrize("extra,reason", [(["--fast"], "--fast"), (["--separable_cbca"], "--separable_cbca"),
                                          (["--arch", "accurate"], "--arch accurate"),
                                          (["--paper_support_regions"], "--paper_support_regions")])
def test_match_refuses_the_grid_where_it_refuses_the_offset(extra, reason, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + ["--vertical_offset", "grid"] + extra)
    assert e.value.code != 0
    assert "--vertical_offset is not available with %s" % reason in capsys.readouterr().err


@pytest.mark.parametrize("flags,text", [(["--vertical_offset_grid", "0x4"], "is not GHxGW with both in [1, 8]"),
                                        (["--vertical_offset_grid", "3x9"], "is not GHxGW with both in [1, 8]"),
                                        (["--vertical_offset", "grid", "--vertical_offset_grid", "four"], "is not GHxGW"),
                                        (["--vertical_offset", "grids"], "nor 'grid'")])
def test_match_refuses_values_outside_the_limits(flags, text, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + flags)
    assert e.value.code != 0 and text in capsys.readouterr().err


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


def test_grid_is_clamped_per_shape(sd):
    # 750 rows at step 8: 94 profiled rows, 8 blocks of 500 columns
    assert sd.vertical_field_grid(750, 500, (3, 4), 8) == (3, 4)
    assert sd.vertical_field_grid(750, 500, (8, 8), 8) == (8, 8)
    assert sd.vertical_field_grid(750, 200, (3, 8), 8) == (3, 4)              # ceil(200 / 64) = 4 blocks
    assert sd.vertical_field_grid(96, 256, (3, 4), 8) == (1, 4)               # 12 profiled rows: one band of >= 8
    assert sd.vertical_field_grid(96, 256, (3, 4), 4) == (3, 4)               # 24: three
    assert sd.vertical_field_grid(128, 192, (3, 3), 4) == (3, 3)
    assert sd.vertical_field_grid(40, 200, (3, 4), 8) == (1, 4)               # 5 profiled rows: never below 1
    assert sd.vertical_field_grid(40, 60, (1, 1), 1) == (1, 1)
    m = sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="grid", vertical_offset_grid=(4, 8), vertical_offset_rows=4))
    assert m.vertical_grid(128, 256) == (4, 4) and m.vertical_grid(40, 200) == (1, 4)


def test_matcher_extras_default_to_nothing_and_the_workspace_grows_by_the_field_only(sd):
    m = sd.StereoMatcher(_StubNet())
    assert m.extras["vertical_offset"] == 0 and m.extras["vertical_offset_grid"] == (3, 4)
    g = sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="grid"))
    assert g.pixel_major() == m.pixel_major() and g.route(40, 48, 16) == m.route(40, 48, 16)
    kernel = m.workspace_cbca_kernel(128, 256, 24)
    auto = sd.workspace_bytes(128, 256, 24, True, kernel, vertical_offset="auto", vertical_offset_rows=4)
    assert sd.workspace_bytes(128, 256, 24, True, kernel, vertical_offset="auto", vertical_offset_rows=4,
                              vertical_offset_grid=(8, 8)) == auto           # the grid means nothing without "grid"
    grid = sd.workspace_bytes(128, 256, 24, True, kernel, vertical_offset="grid", vertical_offset_rows=4)
    assert grid == auto + 3 * 4 * (4 + 8 * 9)
    assert sd.workspace_bytes(128, 256, 24, True, kernel, vertical_offset="grid", vertical_offset_rows=8,
                              vertical_offset_max=8, vertical_offset_grid=(8, 8), pairs_in_flight=2) == \
        2 * (sd.workspace_bytes(128, 256, 24, True, kernel, vertical_offset="auto", vertical_offset_rows=8,
                                vertical_offset_max=8) + 2 * 4 * (4 + 8 * 17))
    sd.StereoMatcher(_StubNet(), hp=dict(cbca_distance=32), confidence=("msm",), views="both", semi_dense="lr",
                     extras=dict(vertical_offset="grid", vertical_offset_grid=(8, 8), vertical_offset_max=8,
                                 vertical_offset_rows=1, vertical_range=4, sgm_independent_directions=True))


@pytest.mark.parametrize("grid", [(0, 4), (3, 9), (3,), (3, 4, 5), "3x4", (3.0, 4), (True, 4), 3])
def test_matcher_refuses_a_grid_outside_the_limits(sd, grid):
    with pytest.raises(ValueError, match=r"vertical_offset_grid must be two integers \(gh, gw\) in \[1, 8\]"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset_grid=grid))
    with pytest.raises(ValueError, match="vertical_offset must be"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="Grid"))


def test_matcher_refuses_the_grid_where_it_refuses_the_offset(sd):
    ex = dict(vertical_offset="grid")
    with pytest.raises(ValueError, match="vertical_offset='grid': the accurate network's decision stage has no row offset"):
        sd.StereoMatcher(_StubAccurateNet(), extras=ex)
    with pytest.raises(ValueError, match="vertical_offset='grid': the matrix-core cost volume"):
        sd.StereoMatcher(_StubNet(), cv_mode=sd.hip.MCCNN_CV_MFMA, extras=ex)
    with pytest.raises(ValueError, match="vertical_offset='grid'.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), layout="plane_major", extras=ex)
    with pytest.raises(ValueError, match="vertical_offset='grid'.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), cbca_order=sd.hip.MCCNN_CBCA_SEPARABLE, extras=ex)
    with pytest.raises(ValueError, match="vertical_offset='grid'.*starts plane-major"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="grid", both_view_support=True))


def test_module_switch_and_the_record(sd):
    import process_functional as pf
    assert pf.VERTICAL_OFFSET == 0 and pf.VERTICAL_OFFSET_GRID == (3, 4) and sd.VERTICAL_FIELD_MAX == 8
    record = sd.vertical_field_record(np.array([1], np.int32), np.array([1, 2, 5], np.int64),
                                      np.array([[1, -1]], np.int32), np.array([[[0, 0, 5], [1, 2, 0]]], np.int64))
    assert record == dict(offset=1, totals=[1, 2, 5], share=0.625, grid=[1, 2], offsets=[[1, -1]],
                          cell_totals=[[[0, 0, 5], [1, 2, 0]]], cell_shares=[[1.0, 1.0 / 3]])
    empty = sd.vertical_field_record([0], [0, 0, 0], [[0]], [[[0, 0, 0]]])
    assert empty["cell_shares"] == [[0.0]] and empty["share"] == 0.0
    # the record of "auto" keeps its keys
    assert sorted(sd.vertical_record([1], [1, 0, 3])) == ["offset", "share", "totals"]


def test_the_grid_chain_is_profile_select_volume_and_nothing_else_changes(sd, monkeypatch):
    """The matcher's cost-volume stage with vertical_offset="grid": the three calls in order, on the workspace's buffers;
    "auto" keeps its own three."""
    import torch
    lib, called = sd.hip.load(), []

    class _Recorder(object):
        def __getattr__(self, name):
            if not name.startswith(("mccnn_vertical_profile", "mccnn_vertical_offset", "mccnn_vertical_field",
                                    "mccnn_cost_volume")) or name == "mccnn_vertical_profile_rows":
                return getattr(lib, name)

            def call(*args):
                called.append(name)
                return 0
            return call

    monkeypatch.setattr(sd.hip, "load", lambda: _Recorder())
    monkeypatch.setattr(sd.hip, "ptr", lambda t: None)
    monkeypatch.setattr(sd.hip, "stream", lambda: None)
    fl = fr = torch.zeros((64, 130, 64))
    hwd = [torch.zeros((64, 130, 8)) for _ in range(4)]

    class _Timer(object):
        def start(self, name):
            pass

        def stop(self):
            pass

    ws = dict(v_offset=torch.zeros(1, dtype=torch.int32), v_totals=torch.zeros(9, dtype=torch.int64),
              v_votes=torch.zeros((8, 3, 9), dtype=torch.int32), v_field=torch.zeros((1, 3), dtype=torch.int32),
              v_cells=torch.zeros((1, 3, 9), dtype=torch.int64))
    sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="grid"))._cost_volumes(fl, fr, 8, hwd, hwd, _Timer(), ws)
    assert called == ["mccnn_vertical_profile", "mccnn_vertical_field_select", "mccnn_cost_volume_field_hwd"]
    del called[:]
    sd.StereoMatcher(_StubNet(), extras=dict(vertical_offset="auto"))._cost_volumes(fl, fr, 8, hwd, hwd, _Timer(), ws)
    assert called == ["mccnn_vertical_profile", "mccnn_vertical_offset_select", "mccnn_cost_volume_offset_hwd"]


# ---- the reason --------------------------------------------------------------------------------------------------------
# (H, W, D, seed, ax, ay, grid): the right image sheared by whole rows about its centre (vertical_field_reference.shear)
SHEARED = [(96, 256, 32, 0, 3, 0, (3, 4)), (96, 256, 32, 1, 3, 0, (3, 4)), (192, 128, 32, 0, 0, 3, (3, 2)),
           (128, 256, 32, 0, 2, 2, (4, 4)), (128, 192, 48, 2, 2, 0, (2, 3)), (128, 192, 48, 2, 2, 0, (3, 3))]
PROFILE = (4, 4)           # max_offset, row_step
_PAIR = {}


def _pair(net_layers, H, W, D, seed):
    """The synthetic pair, its truth, its left features and the aligned and plain results (computed once, never changed)."""
    import oracle as o
    import synthetic
    key = (H, W, D, seed)
    if key not in _PAIR:
        L, R, _, _, truth = synthetic.make_pair(H, W, D, seed=seed)
        c = dict(L=L, R=R, truth=np.asarray(truth, np.float64).reshape(H, W), fl=o.net_features(L, net_layers), runs={})
        c["fr"] = o.net_features(R, net_layers)
        _PAIR[key] = c
    return _PAIR[key]


def _final(c, image, cv, D):
    return ps.match_from_cost_volumes(c["L"], image, cv[0], cv[1], D, True)


def _share(c, final):
    return vr.within_1px(final, c["truth"], margin=6)


@pytest.mark.parametrize("H,W,D,seed,ax,ay,grid", SHEARED)
def test_matching_along_the_field_recovers_a_sheared_pair(net_layers, H, W, D, seed, ax, ay, grid):
    """The whole pipeline on the CPU checker, trained weights, default hyper-parameters, the paper's SGM: the share of
    final pixels within 1 px of the truth (six top and bottom rows left out).  The shear's mean is zero, so the single
    measured offset is 0 and changes nothing; the field exceeds the plain run by more than 0.04 and lies within 0.03 of
    the aligned column.

    Every column of a row is the same chain behind the cost volume, on the same images - the left one and the SHEARED
    right one, which the support regions of the aggregation are cut from - and differs in the cost volume alone.  The
    aligned column takes the volumes of the aligned pair's features: what a perfect correction of the volume would give
    this pair.  (That is how the feature request's table came about: it reads 0.704 for the 128x192 pair, which this
    chain gives and the unsheared pair, at 0.715, does not; the unsheared pair's own share is printed beside it.)

    Measured with the restatement (aligned / plain / vertical_range=2 / field): 0.776 / 0.637 / 0.771 / 0.776 and 0.815 /
    0.710 / 0.811 / 0.813 at 3x4; 0.709 / 0.620 / 0.693 / 0.706 at 3x2; 0.822 / 0.769 / 0.816 / 0.823 at 4x4; 0.704 / 0.612 /
    0.680 / 0.713 at 2x3 and 0.683 at 3x3: field - plain >= 0.054, aligned - field <= 0.021 (the 3x3 grid, whose cells of
    about 700 votes are noisy: its third row band measures -2 -1 0)."""
    import oracle as o
    c = _pair(net_layers, H, W, D, seed)
    if "cv" not in c["runs"]:
        c["runs"]["cv"] = o.compute_cost_volume(c["fl"], c["fr"], D)
        c["runs"]["unsheared"] = _share(c, _final(c, c["R"], c["runs"]["cv"], D))
    moved, dy = vf.shear(c["R"], ax, ay)
    assert abs(float(dy.mean())) < 0.05 and int(dy.max()) == ax + ay == -int(dy.min())
    key = ("sheared", ax, ay)
    if key not in c["runs"]:
        fr = o.net_features(moved, net_layers)
        votes = vo.vertical_profile(c["fl"], fr, D, *PROFILE)
        c["runs"][key] = dict(
            fr=fr, votes=votes,
            aligned=_share(c, _final(c, moved, c["runs"]["cv"], D)),
            plain=_share(c, _final(c, moved, o.compute_cost_volume(c["fl"], fr, D), D)),
            range2=_share(c, _final(c, moved, vr.compute_cost_volume_vertical(c["fl"], fr, D, 2), D)))
    run = c["runs"][key]
    auto = vo.offset_select(run["votes"], PROFILE[0])[0]
    field = vf.field_select(run["votes"], H, PROFILE[1], PROFILE[0], *grid)[0]
    along = _share(c, _final(c, moved, vf.compute_cost_volume_field(c["fl"], run["fr"], D, field, 0), D))
    aligned = run["aligned"]
    print("%dx%dx%d seed %d, ax %d ay %d: aligned %.3f (the unsheared pair %.3f), plain %.3f, auto %.3f (measures %+d), "
          "vertical_range=2 %.3f, field %.3f at %dx%d, cells %s"
          % (H, W, D, seed, ax, ay, aligned, c["runs"]["unsheared"], run["plain"], run["plain"], auto, run["range2"], along,
             grid[0], grid[1], " / ".join(" ".join("%+d" % v for v in row) for row in field)))
    assert auto == 0, (auto, field)
    assert along - run["plain"] > 0.04, (aligned, run["plain"], along)
    assert aligned - along < 0.03, (aligned, run["plain"], along)


def test_an_aligned_pair_measures_zeros_and_keeps_its_map(net_layers):
    import oracle as o
    H, W, D, seed, grid = 96, 256, 32, 0, (3, 4)
    c = _pair(net_layers, H, W, D, seed)
    votes = vo.vertical_profile(c["fl"], c["fr"], D, *PROFILE)
    field = vf.field_select(votes, H, PROFILE[1], PROFILE[0], *grid)[0]
    assert field.shape == grid and not field.any(), field
    plain = _final(c, c["R"], o.compute_cost_volume(c["fl"], c["fr"], D), D)
    along = _final(c, c["R"], vf.compute_cost_volume_field(c["fl"], c["fr"], D, field, 0), D)
    print("%dx%dx%d seed %d, aligned: field all 0, plain %.3f, field %.3f"
          % (H, W, D, seed, _share(c, plain), _share(c, along)))
    assert_bits(np.asarray(along, np.float32), np.asarray(plain, np.float32), "the final map of an aligned pair")
