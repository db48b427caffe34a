"""CPU: what the list loops of match.py share - evaluation.ListScorer (which views of a pair are scored, in which order,
what the running totals take and what the report is told), stereo_device.SaturationRedo (which pairs are repeated) and
the bytes evaluation.ListReport writes.  Recording fakes stand for the evaluators and the sparsifier: every score() and
commit() appends (which, "score" | "commit", id of the map, slot) to one log; no GPU and no torch device is touched."""
import importlib.util
import json
import os

import pytest

import evaluation as ev
from pair_result import PairResult
from conftest import GOLDEN_DIR

_spec = importlib.util.spec_from_file_location("gen_list_report_golden", os.path.join(GOLDEN_DIR, "gen_list_report_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


class FakeScore(object):
    """A PairScore / SparsificationScore whose figures say which call made it."""

    def __init__(self, k):
        self.k = k

    def metrics(self):
        return ev.Metrics.from_result(gen.result_bytes(self.k), gen.THRESHOLDS)

    def figures(self):
        return gen.figures(self.k)


class FakeEvaluator(object):
    thresholds = gen.THRESHOLDS

    def __init__(self, which, log):
        self.which, self.log, self.pairs = which, log, 0

    def score(self, disp, gt, mask=None, slot=0):
        self.log.append((self.which, "score", id(disp), slot))
        return FakeScore(len(self.log))

    def commit(self, disp, gt, mask=None):
        self.log.append((self.which, "commit", id(disp), None))
        self.pairs += 1

    def report(self):
        return ev.Metrics.from_result(gen.result_bytes(0), gen.THRESHOLDS)


class FakeSparsifier(object):
    def __init__(self, log):
        self.log = log

    def score(self, disp, planes, gt):
        self.log.append(("auc", "score", id(disp), None))
        return FakeScore(len(self.log))


class Map(object):
    """Stands for a device tensor: only its identity matters."""


class RecordingReport(ev.ListReport):
    def __init__(self, *evaluators):
        ev.ListReport.__init__(self, *evaluators)
        self.calls = []

    def pair(self, index, name, metrics, path=None, sparsification=None, right=None):
        self.calls.append(("pair", index, name, metrics, sparsification, right))
        ev.ListReport.pair(self, index, name, metrics, path, sparsification=sparsification, right=right)

    def skip(self, index, name):
        self.calls.append(("skip", index, name))
        ev.ListReport.skip(self, index, name)

    def skip_right(self, index, name):
        self.calls.append(("skip_right", index, name))
        ev.ListReport.skip_right(self, index, name)


def _scorer(views="left", sparsifier=False):
    log = []
    left, right = FakeEvaluator("left", log), FakeEvaluator("right", log)
    report = RecordingReport(left, right) if views == "both" else RecordingReport(left)
    return ev.ListScorer(report, FakeSparsifier(log) if sparsifier else None, views), report, log


TRUTH, TRUTH_RIGHT = ("gt", "mask"), ("gt_r", None)


def test_left_only_one_pair(tmp_path):
    scorer, report, log = _scorer()
    m = Map()
    scored = scorer.begin(3, "pair3", TRUTH, TRUTH_RIGHT)        # not --views both: the right truth is ignored
    assert scored.truths == [TRUTH]
    scorer.score(scored, PairResult(m), 0)
    scorer.commit(scored, PairResult(m))
    assert log == [("left", "score", id(m), 0), ("left", "commit", id(m), None)]
    path = tmp_path / "evalMCCNN.json"
    scorer.publish(scored, str(path))
    (kind, index, name, metrics, sparsification, right), = report.calls
    assert (kind, index, name, sparsification, right) == ("pair", 3, "pair3", None, None)
    assert metrics.raw == FakeScore(1).metrics().raw             # of the first entry of the log: that score
    entry = json.loads(path.read_text())
    assert "right" not in entry and "sparsification" not in entry and entry["pair"] == "pair3"


def test_both_views_order_and_commits(tmp_path):
    scorer, report, log = _scorer("both", sparsifier=True)
    maps, planes = [Map(), Map()], [Map(), Map()]
    scored = scorer.begin(0, "pair0", TRUTH, TRUTH_RIGHT)
    scorer.score(scored, PairResult(maps, planes), 1)
    assert log == [("left", "score", id(maps[0]), 1), ("auc", "score", id(maps[0]), None),
                   ("right", "score", id(maps[1]), 1), ("auc", "score", id(maps[1]), None)]
    scorer.commit(scored, PairResult(maps))
    assert log[4:] == [("left", "commit", id(maps[0]), None), ("right", "commit", id(maps[1]), None)]
    scorer.publish(scored, str(tmp_path / "e.json"))
    assert report.calls[-1][4] == gen.figures(2)
    assert report.calls[-1][5]["metrics"].raw == FakeScore(3).metrics().raw
    assert report.calls[-1][5]["sparsification"] == gen.figures(4)
    entry = json.loads((tmp_path / "e.json").read_text())
    assert sorted(entry["right"]) == ["all", "nonocc", "raw", "sparsification"]
    assert not report.left.skipped and not report.right.skipped


def test_both_views_without_right_truth(tmp_path):
    scorer, report, log = _scorer("both", sparsifier=True)
    maps, planes = [Map(), Map()], [Map(), Map()]
    scored = scorer.begin(2, "pair2", TRUTH, None)
    assert report.calls == [("skip_right", 2, "pair2")]
    scorer.score(scored, PairResult(maps, planes), 0)
    scorer.commit(scored, PairResult(maps))
    scorer.publish(scored, str(tmp_path / "e.json"))
    assert all(which != "right" for which, _, _, _ in log)
    assert [e[2] for e in log] == [id(maps[0])] * 3
    assert "right" not in json.loads((tmp_path / "e.json").read_text())
    report.write(str(tmp_path / "eval.json"))
    whole = json.loads((tmp_path / "eval.json").read_text())
    assert "right" not in whole["pairs"][0] and whole["right"]["skipped"] == ["pair2"] and whole["skipped"] == []


@pytest.mark.parametrize("views", ["left", "both"])
def test_without_left_truth_nothing_is_enqueued(views):
    scorer, report, log = _scorer(views, sparsifier=True)
    assert scorer.begin(4, "pair4", None, TRUTH_RIGHT) is None   # a right truth without a left one is ignored
    assert scorer.begin(5, "pair5", None, None) is None
    want = [("skip", 4, "pair4"), ("skip_right", 4, "pair4"), ("skip", 5, "pair5"), ("skip_right", 5, "pair5")]
    assert report.calls == (want if views == "both" else [c for c in want if c[0] == "skip"])
    assert log == []


@pytest.mark.parametrize("views", ["left", "both"])
def test_redo_commits_and_publishes_the_second_score_only(views, tmp_path):
    scorer, report, log = _scorer(views)
    both = views == "both"
    first, redone = ([Map(), Map()], [Map(), Map()]) if both else (Map(), Map())
    scored = scorer.begin(0, "pair0", TRUTH, TRUTH_RIGHT)
    scorer.score(scored, PairResult(first), 0)
    scorer.score(scored, PairResult(redone), 0)
    scorer.commit(scored, PairResult(redone))
    scorer.publish(scored, str(tmp_path / "e.json"))
    ids = lambda maps: [id(m) for m in maps] if both else [id(maps)]      # noqa: E731
    assert [e[1:3] for e in log] == ([("score", i) for i in ids(first)] + [("score", i) for i in ids(redone)]
                                     + [("commit", i) for i in ids(redone)])
    assert not any(kind == "commit" and i in ids(first) for _, kind, i, _ in log)
    n = len(ids(first))
    assert report.calls[-1][3].raw == FakeScore(n + 1).metrics().raw          # the left view's second score
    if both:
        assert report.calls[-1][5]["metrics"].raw == FakeScore(n + 2).metrics().raw
    assert scorer.evaluators[0].pairs == 1 and (not both or scorer.evaluators[1].pairs == 1)


def test_two_slots_five_pairs_commit_in_list_order():
    """The loops' rotation: a pair is scored on its slot when launched and committed when the slot comes round again."""
    scorer, report, log = _scorer()
    maps = [Map() for _ in range(5)]
    pending = []
    for n in range(5):
        if len(pending) == 2:
            scorer.commit(*pending.pop(0))
        scored = scorer.begin(n, "pair%d" % n, TRUTH, None)
        scorer.score(scored, PairResult(maps[n]), n % 2)
        pending.append((scored, PairResult(maps[n])))
    while pending:
        scorer.commit(*pending.pop(0))
    assert [e[2] for e in log if e[1] == "commit"] == [id(m) for m in maps]
    assert [(e[2], e[3]) for e in log if e[1] == "score"] == [(id(m), n % 2) for n, m in enumerate(maps)]
    assert scorer.evaluators[0].pairs == 5


# ---- stereo_device.SaturationRedo --------------------------------------------------------------------------------
class FlagMatcher(object):
    """A matcher whose saturation flag follows a script: flags[k] is what the k-th read returns (and resets)."""

    def __init__(self, flags, checked=True):
        self.flags, self.checked, self.reads = list(flags), checked, 0

    def saturation_checked(self):
        return self.checked

    def features_saturated(self):
        self.reads += 1
        return self.flags[self.reads - 1]

    def saturation_notice(self):
        return "activations left the range: {} repeated"


def _redo(n, flags, checked=True):
    import stereo_device as sd
    built = []
    matchers = [FlagMatcher(flags, checked)] + [FlagMatcher([], checked) for _ in range(n - 1)]
    redo = sd.SaturationRedo(matchers, lambda: built.append("library") or "the library matcher")
    return redo, matchers, built


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("k", [0, 2, 5])
def test_redo_window_is_the_pair_and_the_next_in_flight(n, k):
    redo, matchers, built = _redo(n, [i == k for i in range(8)])
    got = []
    for _ in range(8):
        due = redo.due()
        got.append(due)
        if due:
            assert redo.matcher() == "the library matcher"
    assert got == [k <= i < k + n for i in range(8)]
    assert built == ["library"] and matchers[0].reads == 8
    assert all(m.reads == 0 for m in matchers[1:])               # the flag is shared: the first matcher is asked
    assert redo.notice("out/disp0MCCNN.pfm") == "activations left the range: out/disp0MCCNN.pfm repeated"


def test_redo_flag_inside_the_window_restarts_it():
    redo, _, _ = _redo(2, [False, True, True, False, False, False])
    assert [redo.due() for _ in range(6)] == [False, True, True, True, False, False]
    redo, _, _ = _redo(1, [True, True, False])
    assert [redo.due() for _ in range(3)] == [True, True, False]


@pytest.mark.parametrize("n", [1, 2])
def test_redo_never_reads_a_flag_nobody_raises(n):
    redo, matchers, built = _redo(n, [True] * 4, checked=False)
    assert [redo.due() for _ in range(4)] == [False] * 4
    assert matchers[0].reads == 0 and built == []
    redo, matchers, built = _redo(n, [False] * 4)
    assert [redo.due() for _ in range(4)] == [False] * 4
    assert built == []                                           # no repeat: the library matcher is never built


# ---- evaluation.ListReport ---------------------------------------------------------------------------------------
def test_list_report_writes_the_bytes_on_record(tmp_path):
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    got = gen.scenarios(ev, str(tmp_path))
    assert sorted(got) == sorted(want)
    for scenario in want:
        assert sorted(got[scenario]) == sorted(want[scenario]), scenario
        for name, text in want[scenario].items():
            assert got[scenario][name] == text, "%s: %s" % (scenario, name)
    assert any('"right"' in t for t in want["both"].values()) and not any('"right"' in t for t in want["sparsification"].values())
