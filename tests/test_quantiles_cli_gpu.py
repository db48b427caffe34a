"""GPU: match.py --evaluate --eval_quantiles end to end on files, in the flagless loop, with --pairs_in_flight 2 and with
--pipeline: the three write the same bytes, the quantiles equal the restatement (tests/quantiles_reference.py) applied to
the PFM that was written, and every file of a run with --evaluate alone keeps its bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quantiles_reference as qref
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

H, W, D = 40, 64, 16
PPM = qref.MIDDLEBURY
TAGS = ("A50", "A90", "A95", "A99")
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
FLAGS = ["--evaluate", "--eval_quantiles", "50,90,95,99"]


def _write_pair(dirname, seed):
    from PIL import Image
    import synthetic
    os.makedirs(dirname)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=seed)
    for name, img in (("im0.png", L), ("im1.png", R)):
        g = img[:, :, 0]
        g8 = np.clip((g - g.min()) / (g.max() - g.min()) * 255.0, 0, 255).astype(np.uint8)
        Image.fromarray(g8, mode="L").save(os.path.join(dirname, name))
    with open(os.path.join(dirname, "calib.txt"), "w") as f:
        f.write("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (W, H, D, D))


def _write_truth(dirname, seed, with_mask, view=0):
    """A seeded arbitrary ground truth, about 10 % unknown - the numbers only have to be the restatement's."""
    from PIL import Image
    import util
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.0, D - 1, (H, W)).astype(np.float32)
    gt[rng.random((H, W)) < 0.1] = np.inf
    util.writePfm(gt, os.path.join(dirname, "disp%dGT.pfm" % view))
    if with_mask:
        mask = rng.choice(np.array([0, 128, 255], np.uint8), size=(H, W), p=[0.05, 0.2, 0.75])
        Image.fromarray(mask, mode="L").save(os.path.join(dirname, "mask%dnocc.png" % view))


def _command(lst, data, out, extra):
    return [sys.executable, os.path.join(SRC, "match.py"), "-g", "0", "--list_file", str(lst), "--resume", RESUME,
            "--data_dir", str(data), "--save_dir", str(out), "-t", "e", "-s", "0", "-e", "2"] + extra


def _match(lst, data, out, extra):
    r = subprocess.run(_command(lst, data, out, extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
            for d, _dirs, files in os.walk(root) for f in files}


def _is_eval_json(rel):
    return os.path.basename(rel) in ("eval.json", "evalMCCNN.json")


def _has_key(obj, key):
    if isinstance(obj, dict):
        return key in obj or any(_has_key(v, key) for v in obj.values())
    return isinstance(obj, list) and any(_has_key(v, key) for v in obj)


def _check_block(block, want, n_q=4):
    for r in qref.REGIONS:
        assert block["raw"][r]["n_scored"] == want[r]["n_scored"] and block["raw"][r]["quantile_rank"] == want[r]["rank"]
        assert list(block[r]["quantiles"]) == sorted(TAGS[:n_q])          # (the files are written with sorted keys)
        assert [qref.bits_of(block[r]["quantiles"][t]) for t in TAGS[:n_q]] == want[r]["value"], (r, block[r]["quantiles"])


def _truth(data, rel, view="left"):
    import evaluation as ev
    return ev.load_ground_truth(str(data / rel / "im0.png"), view)


def _pfm(path):
    import util
    return np.asarray(util.readPfm(str(path)), np.float32)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("quantdata")
    data = root / "data"
    rels = ["trainingH/pairA", "trainingH/pairB", "trainingH/pairC"]
    for i, rel in enumerate(rels):
        _write_pair(str(data / rel), seed=90 + i)
    _write_truth(str(data / rels[0]), 1, with_mask=True)
    _write_truth(str(data / rels[1]), 2, with_mask=False)             # the third pair has no ground truth
    lst = root / "list.txt"
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in rels))
    variants = {"eval": ["--evaluate"], "plain": FLAGS, "flight": FLAGS + ["--pairs_in_flight", "2"],
                "pipe": FLAGS + ["--pipeline", "--pairs_in_flight", "2"]}
    for name, extra in variants.items():
        _match(lst, data, root / name, extra)
    return root, data, rels, lst, {name: _files(str(root / name)) for name in variants}


def test_the_three_loops_write_the_same_bytes(runs):
    _root, _data, rels, _lst, files = runs
    base = files["eval"]
    assert sum(_is_eval_json(rel) for rel in base) == 3
    for rel, data in base.items():
        if _is_eval_json(rel):
            assert not _has_key(json.loads(data), "quantiles") and not _has_key(json.loads(data), "quantile_bits"), rel
    for name in ("plain", "flight", "pipe"):
        assert sorted(files[name]) == sorted(base), name
        for rel, data in files[name].items():
            if _is_eval_json(rel):
                assert data == files["plain"][rel], (name, rel)
                assert data != base[rel]
            elif "time" not in os.path.basename(rel).lower():
                assert data == base[rel], (name, rel)                   # maps and every other file: the bytes of --evaluate


def test_values_mean_and_pool_equal_the_restatement(runs):
    root, data, rels, _lst, _files_ = runs
    out = root / "pipe" / "submit_e"
    wants, pool, blocks = [], qref.Pool(), []
    for rel in rels[:2]:
        disp = _pfm(out / rel / "disp0MCCNN.pfm")
        gt, mask = _truth(data, rel)
        want = qref.quantiles(disp, gt, mask, PPM)
        pool.add(disp, gt, mask)
        block = json.loads((out / rel / "evalMCCNN.json").read_text())
        assert block["quantiles"] == [50.0, 90.0, 95.0, 99.0]
        _check_block(block, want)
        wants.append(want)
        blocks.append(block)
    assert wants[0]["nonocc"]["n_scored"] < wants[0]["all"]["n_scored"]
    report = json.loads((out / "eval.json").read_text())
    assert report["quantiles"] == [50.0, 90.0, 95.0, 99.0] and len(report["pairs"]) == 2 and len(report["skipped"]) == 1
    for block, want in zip(report["pairs"], wants):
        _check_block(block, want)
    for r in qref.REGIONS:
        for t in TAGS:
            assert report["mean"][r]["quantiles"][t] == (blocks[0][r]["quantiles"][t] + blocks[1][r]["quantiles"][t]) / 2
    assert report["pooled"]["quantile_bits"] == 16
    _check_block(report["pooled"], pool.pick(PPM))


@pytest.mark.parametrize("extra,message", [
    (["--eval_quantiles", "50"], "--evaluate"),
    (["--evaluate", "--eval_quantiles", "50", "--dataset", "kitti2015"], "kitti2015"),
    (["--evaluate", "--eval_quantiles", "0"], "0 < q <= 100"),
    (["--evaluate", "--eval_quantiles", "101"], "0 < q <= 100"),
    (["--evaluate", "--eval_quantiles", "1,2,3,4,5,6,7,8,9"], "1 to 8"),
], ids=["no_evaluate", "kitti", "zero", "above_100", "nine"])
def test_refusals(runs, tmp_path, extra, message):
    _root, data, _rels, lst, _files_ = runs
    r = subprocess.run(_command(lst, data, tmp_path / "o", extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 2 and "--eval_quantiles" in text and message in text, text[-2000:]
    assert not (tmp_path / "o").exists()


def test_views_both_scores_the_right_map(runs, tmp_path):
    import shutil
    _root, data, rels, _lst, _files_ = runs
    d2 = tmp_path / "data"
    shutil.copytree(str(data / rels[0]), str(d2 / "p"))
    _write_truth(str(d2 / "p"), 7, with_mask=True, view=1)
    lst = tmp_path / "list.txt"
    lst.write_text("%s/im0.png\n" % (d2 / "p"))
    cmd = _command(lst, d2, tmp_path / "o", ["--evaluate", "--eval_quantiles", "99,50", "--views", "both"])
    cmd[cmd.index("-e") + 1] = "0"
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    out = tmp_path / "o" / "submit_e"
    block = json.loads((out / "p" / "evalMCCNN.json").read_text())
    ppm = (990000, 500000)
    for view, name, got in (("left", "disp0MCCNN.pfm", block), ("right", "disp1MCCNN.pfm", block["right"])):
        gt, mask = _truth(d2, "p", view)
        want = qref.quantiles(_pfm(out / "p" / name), gt, mask, ppm)
        for r_ in qref.REGIONS:
            assert got["raw"][r_]["n_scored"] == want[r_]["n_scored"] and got["raw"][r_]["quantile_rank"] == want[r_]["rank"]
            assert [qref.bits_of(got[r_]["quantiles"][t]) for t in ("A99", "A50")] == want[r_]["value"]
    report = json.loads((out / "eval.json").read_text())
    assert report["right"]["pooled"]["quantile_bits"] == 16 and "A99" in report["right"]["mean"]["all"]["quantiles"]
