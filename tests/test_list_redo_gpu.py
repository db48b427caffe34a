"""GPU: the saturation redo together with scoring, in the three list loops of match.py (flagless, --pairs_in_flight 2,
--pipeline), on the three-pair 48 x 64 x 16 tree of test_right_view_cli_gpu.py with --evaluate --views both
--confidence mmn,lrc --eval_quantiles 50,90.  With the matchers' saturation flag patched to be always up every pair is
matched by the split-operand kernels, discarded, repeated with the library convolutions, scored again and committed
once; a fourth, unpatched run with --features library writes what the redo matcher computes without the redo path.  All
four write the same bytes - maps, planes, every evalMCCNN.json and eval.json with its pooled totals and pooled
quantiles: a total that had taken a discarded map, or pairs out of list order, would differ."""
import contextlib
import io

import pytest

from test_right_view_cli_gpu import LOOPS, RESUME, _files, tree  # noqa: F401  (the fixture and its tree)

pytestmark = pytest.mark.gpu

FLAGS = ["--evaluate", "--views", "both", "--confidence", "mmn,lrc", "--eval_quantiles", "50,90"]
NOTICE = "repeated with the float32 library convolutions"


def _main(tree, name, extra):  # noqa: F811
    """match.main in this process (no -g: the visible GPU stands) -> (files but the time files, what it printed)."""
    import match
    root = tree["root"]
    argv = ["--list_file", str(root / "mb.txt"), "--resume", RESUME, "--data_dir", str(root / "mb"),
            "--save_dir", str(root / ("redo_" + name)), "-t", "v", "-s", "0", "-e", "2"] + FLAGS + extra
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        match.main(argv)
    return _files(root / ("redo_" + name)), log.getvalue()


@pytest.fixture(scope="module")
def runs(tree):  # noqa: F811
    import stereo_device as sd
    out = {"library": _main(tree, "library", ["--features", "library"])}
    patch = pytest.MonkeyPatch()
    patch.setattr(sd.StereoMatcher, "saturation_checked", lambda self: True)
    patch.setattr(sd.StereoMatcher, "features_saturated", lambda self, reset=True: True)
    try:
        for name, extra in LOOPS:
            out[name] = _main(tree, name, extra)
    finally:
        patch.undo()
    return out


def test_every_pair_is_repeated_once(runs):
    assert runs["library"][1].count(NOTICE) == 0
    for name, _ in LOOPS:
        assert runs[name][1].count(NOTICE) == 3, runs[name][1][-3000:]


def test_redone_lists_write_the_bytes_of_the_library_run(runs):
    want = runs["library"][0]
    assert sum(f.endswith("evalMCCNN.json") for f in want) == 3 and sum(f.endswith("eval.json") for f in want) == 1
    assert sum(f.endswith(".pfm") for f in want) == 3 * (2 + 2 * 2)        # per pair: two maps, two planes per view
    for name, _ in LOOPS:
        got = runs[name][0]
        assert sorted(got) == sorted(want), name
        for f in want:
            assert got[f] == want[f], "%s: %s differs from the --features library run" % (name, f)
