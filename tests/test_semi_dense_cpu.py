"""CPU: what the semi-dense maps promise without a GPU - the restatement (tests/semi_dense_reference.py) against a second,
independent statement of the components; SemiDenseRule's text form and refusals; every argument refusal of
mccnn_semi_dense_select / mccnn_speckle_filter (validation runs before any HIP call); StereoMatcher's defaults; and why
the feature exists: on synthetic pairs the kept pixels of `lr,speckle:20:1` are more often right than the dense map's."""
import ctypes
import os

import numpy as np
import pytest

import semi_dense_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED, E_SCRATCH = -1, -2, -3


@pytest.mark.parametrize("seed", range(6))
def test_flood_fill_agrees_with_scipy_on_quantised_maps(seed):
    """max_diff = 0 makes "linked" mean "equal value": scipy.ndimage.label per value is the same partition."""
    disp = ref.random_map(40, 56, seed, levels=2 + seed % 3)
    sizes = ref.component_sizes(disp, 0.0)
    assert np.array_equal(sizes, ref.component_sizes_equal_values(disp))
    assert (sizes[~ref.valid(disp)] == 0).all() and (sizes[ref.valid(disp)] >= 1).all() and sizes.max() > 4
    # levels one apart with max_diff below one: the same partition again; at one and above, components only merge
    assert np.array_equal(ref.component_sizes(disp, 0.5), sizes)
    assert (ref.component_sizes(disp, 1.0) >= sizes).all() and (ref.component_sizes(disp, np.inf) >= sizes).all()
    out, _ = ref.speckle_filter(disp, 3, 0.0)
    assert np.array_equal(ref.bits(out)[sizes >= 3], ref.bits(disp)[sizes >= 3]) and (out[sizes < 3] == np.inf).all()


def test_restatement_details():
    assert ref.valid(np.float32(-0.0)) and ref.valid(np.float32(0)) and ref.valid(np.float32(3.4e38))
    for v in (-1.0, np.nan, np.inf, -np.inf, -1e-45):
        assert not ref.valid(np.float32(v))
    assert ref.linked(0.0, 1.0, 1.0) and not ref.linked(0.0, np.nextafter(np.float32(1), np.float32(2)), 1.0)
    assert ref.linked(-0.0, 0.0, 0.0) and not ref.linked(0.0, np.nan, np.inf) and ref.linked(0.0, 3e38, np.inf)
    ramp = np.arange(12, dtype=np.float32).reshape(1, 12)
    assert (ref.component_sizes(ramp, 1.0) == 12).all() and (ref.component_sizes(ramp, 0.5) == 1).all()
    board = ((np.arange(6)[:, None] + np.arange(7)[None, :]) % 2).astype(np.float32)
    assert (ref.component_sizes(board, 0.0) == 1).all(), "diagonal neighbours never link"
    disp = np.array([[1.0, -1.0, np.nan, 2.0, -0.0]], np.float32)
    planes = np.array([[[5.0, 5.0, 5.0, np.nan, -np.inf]]], np.float32)
    status = np.array([[0, 0, 0, 0, 2]], np.int32)
    got = ref.select(disp, status, planes, ("mmn",), {"mmn": 5.0}, True)
    assert np.array_equal(ref.bits(got), ref.bits(np.array([[1.0, np.inf, np.inf, np.inf, np.inf]], np.float32)))
    got = ref.select(disp, None, planes, ("mmn",), {"mmn": -np.inf})
    assert np.array_equal(ref.bits(got), ref.bits(np.array([[1.0, np.inf, np.inf, np.inf, -0.0]], np.float32)))


def test_rule_parsing_and_refusals():
    import stereo_device as sd
    R = sd.SemiDenseRule
    r = R.parse(" lr , speckle:20:1")
    assert r.require_match and r.thresholds == {} and r.speckle == (20, 1.0) and r.measures == ()
    assert R.parse("speckle:7").speckle == (7, 1.0) and R.parse("speckle:7:inf").speckle == (7, float("inf"))
    r = R.parse("lrc:-1,mmn:0.1,speckle:3:0")
    assert r.measures == ("mmn", "lrc") and not r.require_match and r.speckle == (3, 0.0)
    assert r.thresholds["mmn"] == float(np.float32(0.1)) != 0.1, "floats are rounded to float32 once"
    assert R.parse(r.describe()) == r and R.parse(r) is r and r.describe() == R.parse("mmn:0.1,lrc:-1,speckle:3:0.0").describe()
    assert R(True, {"cur": 2}, (4, 0.5)) == R.parse("cur:2,speckle:4:0.5,lr")
    assert R.parse("msm:-inf").thresholds == {"msm": float("-inf")}
    for bad in ("", " ", ",", "lr,", "lr,lr", "mmn:1,mmn:2", "speckle:3,speckle:4", "mmn:nan", "speckle:3:nan", "speckle:3:-0.5",
                "speckle:0", "speckle:-2", "speckle:2.5", "speckle", "speckle:", "speckle:3:1:2", "pkr:1", "MMN:1", "mmn", "mmn:",
                "mmn:x", "lr:1", "lrc"):
        with pytest.raises(ValueError):
            R.parse(bad)
    for bad in (dict(), dict(thresholds={"pkr": 1.0}), dict(thresholds={"mmn": float("nan")}), dict(speckle=(0, 1.0)),
                dict(speckle=(3, -1.0)), dict(speckle=(3, float("nan")))):
        with pytest.raises(ValueError):
            R(**bad)
    with pytest.raises(ValueError):
        R.parse(None)


def test_argument_refusals():
    import _hipabi
    lib = _hipabi.load()
    assert lib.mccnn_version() == 7 == _hipabi.MCCNN_ABI_VERSION
    p = ctypes.c_void_p
    disp, status, planes, out, sizes, scratch = (p(a) for a in (0x100000, 0x200000, 0x300000, 0x900000, 0xA00000, 0xB00000))
    st = None
    H, W = 4, 6
    plane = H * W * 4

    def msg():
        return lib.mccnn_last_error_string()

    sel = lib.mccnn_semi_dense_select
    mc = (ctypes.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    who = b"mccnn_semi_dense_select"
    assert sel(None, status, planes, H, W, 15, 3, mc, 1, out, st) == E_INVALID and b"null pointer" in msg() and who in msg()
    assert sel(disp, status, planes, H, W, 15, 3, mc, 1, None, st) == E_INVALID and b"null pointer" in msg()
    for h, w in ((0, 6), (4, 0), (-1, 6), (4, -1)):
        assert sel(disp, status, planes, h, w, 15, 3, mc, 1, out, st) == E_INVALID and b"non-positive" in msg()
    for have, use in ((16, 0), (15, 16), (0x80000000, 0), (31, 17)):
        assert sel(disp, status, planes, H, W, have, use, mc, 1, out, st) == E_INVALID and b"above 15" in msg()
    for have, use in ((0, 1), (1, 2), (5, 7), (14, 15), (8, 4)):
        assert sel(disp, status, planes, H, W, have, use, mc, 1, out, st) == E_INVALID and b"subset" in msg()
    assert sel(disp, status, None, H, W, 15, 1, mc, 1, out, st) == E_INVALID and b"planes" in msg()
    assert sel(disp, status, planes, H, W, 15, 1, None, 1, out, st) == E_INVALID and b"min_conf" in msg()
    assert sel(disp, None, planes, H, W, 15, 3, mc, 1, out, st) == E_INVALID and b"require_match" in msg()
    for b in range(4):
        bad = (ctypes.c_float * 4)(0, 0, 0, 0)
        bad[b] = float("nan")
        assert sel(disp, status, planes, H, W, 15, 1 << b, bad, 0, out, st) == E_INVALID and b"NaN" in msg()
    for off in (0, 4, plane - 4, 4 - plane):
        assert sel(disp, status, planes, H, W, 15, 3, mc, 1, p(disp.value + off), st) == E_INVALID and b"overlaps disp" in msg()
        assert sel(disp, status, planes, H, W, 15, 3, mc, 1, p(status.value + off), st) == E_INVALID and b"overlaps status" in msg()
    for k, have in ((1, 2), (2, 3), (4, 15)):
        for o in (planes.value, planes.value + k * plane - 4, planes.value - plane + 4):
            assert sel(disp, status, planes, H, W, have, 2, mc, 1, p(o), st) == E_INVALID and b"overlaps planes" in msg()

    spk = lib.mccnn_speckle_filter
    nbytes = lib.mccnn_speckle_scratch_bytes
    who = b"mccnn_speckle_filter"
    need = nbytes(H, W)
    assert need == 2 * plane and nbytes(0, 5) == 0 and nbytes(5, -1) == 0 and nbytes(65536, 32768) == 0
    assert nbytes(46341, 46340) == 2 * 4 * 46341 * 46340 and nbytes(1, 2 ** 31 - 1) == 8 * (2 ** 31 - 1)
    assert spk(None, H, W, 1.0, 1, out, sizes, scratch, need, st) == E_INVALID and b"null pointer" in msg() and who in msg()
    assert spk(disp, H, W, 1.0, 1, out, sizes, None, need, st) == E_INVALID and b"null pointer" in msg()
    assert spk(disp, H, W, 1.0, 1, None, None, scratch, need, st) == E_INVALID and b"both null" in msg()
    for h, w in ((0, 6), (4, 0), (-1, 6), (4, -1)):
        assert spk(disp, h, w, 1.0, 1, out, sizes, scratch, need, st) == E_INVALID and b"non-positive" in msg()
    for bad in (float("nan"), -1.0, -1e-45, float("-inf")):
        assert spk(disp, H, W, bad, 1, out, sizes, scratch, need, st) == E_INVALID and b"max_diff" in msg()
    assert spk(disp, H, W, 1.0, 0, out, sizes, scratch, need, st) == E_INVALID and b"min_size" in msg()
    assert spk(disp, 65536, 32768, 1.0, 1, out, sizes, scratch, 1 << 40, st) == E_UNSUPPORTED and b"pixels" in msg()
    assert spk(disp, H, W, 1.0, 1, out, sizes, scratch, need - 1, st) == E_SCRATCH and b"mccnn_speckle_scratch_bytes" in msg()
    assert spk(disp, H, W, 1.0, 1, out, sizes, scratch, 0, st) == E_SCRATCH
    for off in (4, 8, 12):
        assert spk(disp, H, W, 1.0, 1, out, sizes, p(scratch.value + off), need, st) == E_SCRATCH and b"aligned" in msg()
    for off in (0, 4, plane - 4, 4 - plane):
        assert spk(disp, H, W, 1.0, 1, p(disp.value + off), sizes, scratch, need, st) == E_INVALID and b"overlaps" in msg()
        assert spk(disp, H, W, 1.0, 1, out, p(disp.value + off), scratch, need, st) == E_INVALID and b"overlaps" in msg()
        assert spk(disp, H, W, 1.0, 1, out, p(out.value + off), scratch, need, st) == E_INVALID and b"overlaps" in msg()
    for other in (disp, out, sizes):
        for off in (0, 16 - need, plane - 16):
            assert spk(disp, H, W, 1.0, 1, out, sizes, p(other.value + off), need, st) == E_INVALID and b"scratch" in msg()


def test_header_states_the_definitions():
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    for phrase in ("0x7F800000", "finite and >= 0", "fabsf(disp[p] - disp[q]) <= max_diff", "speckle_filter(select(map))",
                   "mccnn_speckle_scratch_bytes(H, W)", "diagonal neighbours"):
        assert phrase in text, phrase


class _StubNet(object):
    def supports_split_features(self):
        return True


def test_matcher_defaults_unchanged(monkeypatch):
    import inspect
    import torch
    import stereo_device as sd
    monkeypatch.setattr(sd.hip, "require_device", lambda: torch.device("cpu"))
    m = sd.StereoMatcher(_StubNet())
    assert m.semi_dense is None and m.confidence == () and m.views == "left"
    sig = inspect.signature(sd.StereoMatcher.__init__)
    assert sig.parameters["semi_dense"].default is None
    for entry in ("match", "match_u8"):
        assert inspect.signature(getattr(sd.StereoMatcher, entry)).parameters["semi_out"].default is None
    with pytest.raises(ValueError, match="mmn"):
        sd.StereoMatcher(_StubNet(), semi_dense="lr,mmn:0.5")
    with pytest.raises(ValueError, match="cur"):
        sd.StereoMatcher(_StubNet(), confidence=("mmn", "lrc"), semi_dense="mmn:0.5,cur:1")
    ok = sd.StereoMatcher(_StubNet(), confidence=("lrc", "mmn"), semi_dense="lrc:-1,speckle:9")
    assert ok.semi_dense == sd.SemiDenseRule.parse("speckle:9:1,lrc:-1") and ok.confidence == ("mmn", "lrc")
    assert sd.StereoMatcher(_StubNet(), semi_dense=sd.SemiDenseRule(True)).semi_dense.describe() == "lr"
    H, W, D = 40, 48, 16
    base = sd.workspace_bytes(H, W, D)
    assert sd.workspace_bytes(H, W, D, semi_dense=False) == base
    assert sd.workspace_bytes(H, W, D, semi_dense=True) == base + 5 * H * W * 4
    assert (sd.workspace_bytes(H, W, D, views="both", confidence=2, semi_dense=True, pairs_in_flight=3)
            == 3 * (sd.workspace_bytes(H, W, D, views="both", confidence=2) + 10 * H * W * 4))
    assert sd.PostView(*range(11)).semi is None


@pytest.mark.parametrize("H,W,D,seed", [(96, 128, 32, 0), (96, 128, 32, 1), (128, 192, 48, 2)])
def test_semi_dense_beats_the_dense_map_on_synthetic_pairs(net_layers, H, W, D, seed):
    """The whole pipeline on the CPU checker, trained weights, default hyper-parameters, the rule lr,speckle:20:1: among the
    kept pixels the share with an error above 1 px, and above 2 px, is lower than over the dense map, and between half
    and 95 % of the pixels are kept.  The ordering and that band are asserted; the figures are printed.  As measured when
    the feature was proposed (density, bad 1 px kept / dense, bad 2 px kept / dense):
        96x128x32 seed 0   0.780  0.267 / 0.314  0.215 / 0.250
        96x128x32 seed 1   0.808  0.279 / 0.359  0.191 / 0.249
        128x192x48 seed 2  0.774  0.336 / 0.375  0.318 / 0.341"""
    import oracle as o
    import stereo_device as sd
    import synthetic
    L, R, _, _, truth = synthetic.make_pair(H, W, D, seed=seed)
    dense, stages = o.match_pair(L, R, D, net_layers, return_all=True)
    status = o.lr_status(stages["wta"][0], stages["wta"][1], D)
    rule = sd.SemiDenseRule.parse("lr,speckle:20:1")
    sparse = ref.semi_dense(dense, rule, status)
    kept = ref.valid(sparse)
    assert np.array_equal(ref.bits(sparse)[kept], ref.bits(dense)[kept]) and (sparse[~kept] == np.inf).all()
    err = np.abs(dense.astype(np.float64) - np.asarray(truth, np.float64).reshape(H, W))
    density = float(kept.mean())
    figures = [(float((err[kept] > t).mean()), float((err > t).mean())) for t in (1.0, 2.0)]
    print("%dx%dx%d seed %d: density %.3f, bad 1 px %.3f kept / %.3f dense, bad 2 px %.3f kept / %.3f dense"
          % ((H, W, D, seed, density) + figures[0] + figures[1]))
    assert 0.5 <= density <= 0.95, density
    for kept_share, dense_share in figures:
        assert kept_share < dense_share, figures


# ---- match.py --semi_dense and the list report -------------------------------------------------------------------------
BASE_ARGS = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]


def test_match_parser_accepts_the_flag_and_it_is_off_by_default(capsys):
    import match
    assert match.parser.parse_args(BASE_ARGS).semi_dense is None
    args = match.parser.parse_args(BASE_ARGS + ["--semi_dense", "lr,speckle:20:1", "--pipeline", "--views", "both"])
    assert args.semi_dense == "lr,speckle:20:1"
    # refused before the GPU is looked for: a KITTI data set, a measure --confidence lacks, a rule that does not parse
    for extra, text in ((["--dataset", "kitti2015", "--semi_dense", "lr"], "--semi_dense is not available with --dataset kitti2015"),
                        (["--dataset", "kitti2012", "--semi_dense", "lr"], "--semi_dense is not available with --dataset kitti2012"),
                        (["--semi_dense", "lr,mmn:0.5"], "confidence measure mmn"),
                        (["--confidence", "mmn", "--semi_dense", "mmn:0.5,cur:1"], "confidence measure cur"),
                        (["--semi_dense", "speckle:0"], "--semi_dense: "), (["--semi_dense", ""], "--semi_dense: ")):
        with pytest.raises(SystemExit) as e:
            match.main(BASE_ARGS + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err


def _metrics(ev, n_valid, n_invalid, n_bad):
    raw = dict((r, dict(n_valid=n_valid, n_invalid=n_invalid, n_bad=list(n_bad), sum_abs=1.5, sum_sq=4.5)) for r in ev.REGIONS)
    return ev.Metrics(raw, (1.0, 2.0))


def test_semi_dense_block_and_report_keys(tmp_path):
    import json
    import evaluation as ev
    block = ev.semi_dense_block(_metrics(ev, 200, 50, (30, 15)), "lr")
    assert block["rule"] == "lr" and block["density"] == {"all": 75.0, "nonocc": 75.0}
    assert block["bad_of_scored"]["all"] == {"1.0": 20.0, "2.0": 10.0} and block["all"]["invalid"] == 25.0
    assert block["all"]["bad"] == {"1.0": 40.0, "2.0": 32.5}, "the dense figures count dropped pixels as bad"
    empty = ev.semi_dense_block(_metrics(ev, 40, 40, (0, 0)))
    assert "rule" not in empty and empty["density"]["all"] == 0.0 and empty["bad_of_scored"]["all"] == {"1.0": None, "2.0": None}
    none = ev.semi_dense_block(_metrics(ev, 0, 0, (0, 0)))
    assert none["density"]["all"] is None

    class Total(object):
        thresholds = (1.0, 2.0)

        def __init__(self, m):
            self.m = m

        def report(self):
            return self.m

    dense, sparse = _metrics(ev, 200, 0, (60, 40)), _metrics(ev, 200, 50, (30, 15))
    for semi in (None, ("lr", Total(sparse), None)):
        report = ev.ListReport(Total(dense), **(dict(semi=semi) if semi else {}))
        path = tmp_path / ("pair_%s.json" % bool(semi))
        report.pair(0, "pair0", dense, str(path), **(dict(semi_dense=[sparse]) if semi else {}))
        report.write(str(tmp_path / ("list_%s.json" % bool(semi))))
        entry = json.loads(path.read_text())
        whole = json.loads((tmp_path / ("list_%s.json" % bool(semi))).read_text())
        if not semi:
            assert "semi_dense" not in entry and "semi_dense" not in whole and "semi_dense" not in whole["pairs"][0]
            plain = (path.read_text(), (tmp_path / "list_False.json").read_text())
            continue
        assert entry["semi_dense"] == ev.semi_dense_block(sparse, "lr") == whole["pairs"][0]["semi_dense"]
        assert sorted(whole["semi_dense"]) == ["mean", "pooled", "rule"]
        assert whole["semi_dense"]["pooled"] == ev.semi_dense_block(sparse)
        assert whole["semi_dense"]["mean"]["density"] == {"all": 75.0, "nonocc": 75.0}
        entry.pop("semi_dense"), whole.pop("semi_dense"), whole["pairs"][0].pop("semi_dense")
        assert json.dumps(entry, indent=1, sort_keys=True) + "\n" == plain[0], "every other key keeps its bytes"
        assert json.dumps(whole, indent=1, sort_keys=True) + "\n" == plain[1]


def _load_report_golden():
    """tests/golden/gen_list_report_golden.py, loaded the way tests/test_list_scoring_cpu.py loads it."""
    import importlib.util
    from conftest import GOLDEN_DIR
    spec = importlib.util.spec_from_file_location("gen_list_report_golden", os.path.join(GOLDEN_DIR, "gen_list_report_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _strip_semi(obj):
    """(the object without any "semi_dense" key at any depth, the paths at which one was found)."""
    found = []

    def walk(o, path):
        if isinstance(o, dict):
            found.extend(path + ("semi_dense",) for k in o if k == "semi_dense")
            return dict((k, walk(v, path + (k,))) for k, v in o.items() if k != "semi_dense")
        if isinstance(o, list):
            return [walk(v, path + (n,)) for n, v in enumerate(o)]
        return o
    return walk(obj, ()), found


def test_list_reports_keep_the_bytes_on_record_without_and_under_the_flag(tmp_path):
    """The goldens of tests/test_list_scoring_cpu.py, reused and not edited.  Without the flag the scripted scenarios
    (left only, described, nothing scored, sparsification, both views with a skipped right view and a repeated pair,
    quantiles) still write the texts on record.  With it - the same scenarios through a ListReport that is given
    semi=(rule, evaluator, evaluator) and a sparse map's Metrics for every scored view of every pair - every file has its
    "semi_dense" blocks where they belong, and without them it is the text on record, byte for byte."""
    import json
    import types
    import evaluation as ev
    gen = _load_report_golden()
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    plain_dir, flag_dir = tmp_path / "plain", tmp_path / "flag"
    plain_dir.mkdir(), flag_dir.mkdir()
    assert gen.scenarios(ev, str(plain_dir)) == want
    assert not any('"semi_dense"' in text for texts in want.values() for text in texts.values())

    rule = "lr,speckle:20:1.0"

    def sparse(k):
        return ev.Metrics.from_result(gen.result_bytes(k), gen.THRESHOLDS)

    class SparseTotal(object):
        thresholds = gen.THRESHOLDS

        def __init__(self, k):
            self.k = k

        def report(self):
            return sparse(self.k)

    class FlaggedReport(ev.ListReport):
        def __init__(self, evaluator, right_evaluator=None):
            ev.ListReport.__init__(self, evaluator, right_evaluator,
                                   semi=(rule, SparseTotal(9), SparseTotal(0) if right_evaluator is not None else None))

        def pair(self, index, name, metrics, path=None, sparsification=None, right=None):
            views = [sparse(index + 1)] + ([sparse(index)] if right is not None else [])     # (index 0, right: empty nonocc)
            ev.ListReport.pair(self, index, name, metrics, path, sparsification=sparsification, right=right, semi_dense=views)

    flagged = types.SimpleNamespace(**dict((k, getattr(ev, k)) for k in dir(ev) if not k.startswith("__")))
    flagged.ListReport = FlaggedReport
    got = gen.scenarios(flagged, str(flag_dir))
    assert sorted(got) == sorted(want)
    for scenario in want:
        assert sorted(got[scenario]) == sorted(want[scenario]), scenario
        both = scenario.startswith("both") or scenario == "quantiles_both"
        for name, text in want[scenario].items():
            stripped, found = _strip_semi(json.loads(got[scenario][name]))
            assert json.dumps(stripped, indent=1, sort_keys=True) + "\n" == text, "%s: %s" % (scenario, name)
            record = json.loads(text)
            if name != "eval.json":
                # a pair's file: the left block, and the right one exactly where the right view was scored
                assert found == [("semi_dense",)] + ([("right", "semi_dense")] if "right" in record else []), (scenario, name)
                assert json.loads(got[scenario][name])["semi_dense"]["rule"] == rule
                continue
            expect = [("semi_dense",)] + ([("right", "semi_dense")] if both else [])
            for n, p in enumerate(record["pairs"]):
                expect.append(("pairs", n, "semi_dense"))
                if "right" in p:
                    expect.append(("pairs", n, "right", "semi_dense"))
            assert sorted(found, key=repr) == sorted(expect, key=repr), (scenario, name)
            whole = json.loads(got[scenario][name])
            assert whole["semi_dense"]["rule"] == rule and whole["semi_dense"]["pooled"] == ev.semi_dense_block(sparse(9))
            blocks = [p["semi_dense"] for p in whole["pairs"]]
            assert all(b == ev.semi_dense_block(sparse(p["index"] + 1), rule) for b, p in zip(blocks, whole["pairs"]))
            if blocks:
                assert whole["semi_dense"]["mean"]["density"]["all"] == sum(b["density"]["all"] for b in blocks) / len(blocks)
            else:
                assert whole["semi_dense"]["mean"]["density"] == {"all": None, "nonocc": None}
            if both:
                right = [p["right"]["semi_dense"] for p in whole["pairs"] if "right" in p]
                assert whole["right"]["semi_dense"]["pooled"] == ev.semi_dense_block(sparse(0))
                assert whole["right"]["semi_dense"]["mean"]["density"]["all"] == (
                    sum(b["density"]["all"] for b in right) / len(right) if right else None)


def test_split_result():
    """pair_result.PairResult: the public shape of every combination, and its inverse by configuration."""
    from pair_result import PairResult
    for both in (False, True):
        lead = (2,) if both else ()
        m, p, s = np.zeros(lead + (3, 4)), np.zeros(lead + (2, 3, 4)), np.ones(lead + (3, 4))
        for has_p in (False, True):
            for has_s in (False, True):
                record = PairResult(m, p if has_p else None, s if has_s else None)
                public = record.public()
                if not (has_p or has_s):
                    assert public is m
                else:
                    want = (m,) + ((p,) if has_p else ()) + ((s,) if has_s else ())
                    assert isinstance(public, tuple) and len(public) == len(want)
                    assert all(a is b for a, b in zip(public, want))
                got = PairResult.decode(public, has_p, has_s)
                assert all(a is b for a, b in zip(got, record)) and (got.planes is None) == (not has_p)
                # one view: index v of every present field under views="both", the record itself otherwise
                for v in range(2 if both else 1):
                    view = record.view(v, both)
                    if not both:
                        assert view is record
                    else:
                        assert np.shares_memory(view.map, m[v]) and view.map.shape == (3, 4)
                        assert (view.planes is None) == (not has_p) and (view.sparse is None) == (not has_s)
                        assert not has_p or view.planes.shape == (2, 3, 4)
                applied = record.apply(lambda t: t + 1)
                assert [t is None for t in applied] == [t is None for t in record] and (applied.map == 1).all()
    both = np.zeros((2, 3, 4))
    assert PairResult.decode((both, np.zeros((2, 2, 3, 4)), both), True, True).sparse is both
    # what no rule on dimensions can tell: a planes tensor and a sparse tensor of equal ndim (and of the map's)
    planes, sparse = np.zeros((2, 3, 4)), np.ones((2, 3, 4))
    got = PairResult.decode((both, planes, sparse), True, True)
    assert got.map is both and got.planes is planes and got.sparse is sparse
    got = PairResult.decode((both, planes), True, False)
    assert got.planes is planes and got.sparse is None
    got = PairResult.decode((both, sparse), False, True)
    assert got.planes is None and got.sparse is sparse
