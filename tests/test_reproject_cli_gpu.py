"""GPU: match.py --depth --point_cloud on files, in the three list loops (flagless, --pairs_in_flight 2, --pipeline), on a
two-pair Middlebury tree at 48 x 64 x 16 whose two calib.txt differ: the loops write the same bytes, depth0MCCNN.pfm and
points0MCCNN.ply equal the restatement (tests/reproject_reference.py) applied to the written disp0MCCNN.pfm under each
pair's own calibration, and every other file is that of a run without the flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reproject_reference as ref
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

H, W, D = 48, 64, 16
MAX_DEPTH = 120000.0     # pair 1: Z = 930 363 / d, so disparities under 7.75 px are no points; pair 0 keeps every pixel
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
# (fx, fy, cx, cy, baseline, doffs) of the two pairs; the second file lists its keys in another order
CALIBS = ((3997.684, 3990.25, 30.5, 22.25, 193.001, 12.5), (1733.74, 1733.74, 31.0, 24.0, 536.62, 0.0))
TEXTS = ("cam0=[%r 0 %r; 0 %r %r; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=%r\nbaseline=%r\nwidth=%d\nheight=%d\nndisp=%d\n"
         "isint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n",
         # (util.parseCalib reads the size from lines 4 to 6 by position, as the reference does: they stay there)
         "baseline=%r\ndoffs=%r\ncam1=[1 0 0; 0 1 0; 0 0 1]\nisint=0\nwidth=%d\nheight=%d\nndisp=%d\ncam0=[%r 0 %r; 0 %r %r; 0 0 1]\n"
         "vmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")
LOOPS = (("plain", []), ("two", ["--pairs_in_flight", "2"]), ("pipe", ["--pipeline"]))
FLAGS = ["--depth", "--point_cloud", "--max_depth", MAX_DEPTH]
NEW = ("depth0MCCNN.pfm", "points0MCCNN.ply")


def _run(lst, data, out, n, extra):
    cmd = [sys.executable, os.path.join(SRC, "match.py"), "-g", "0", "--list_file", str(lst), "--resume", RESUME,
           "--data_dir", str(data), "--save_dir", str(out), "-t", "v", "-s", "0", "-e", str(n - 1)] + [str(a) for a in extra]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)


def _files(root):
    out = {}
    for dirpath, _dirs, names in os.walk(str(root)):
        for name in names:
            if name != "timeMCCNN.txt":
                rel = os.path.relpath(os.path.join(dirpath, name), str(root))
                out[rel] = open(os.path.join(dirpath, name), "rb").read()
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from PIL import Image
    import synthetic
    root = tmp_path_factory.mktemp("geometry")
    mb = root / "mb" / "trainingG"
    greys = []
    for i in range(2):
        _, _, left, right, _ = synthetic.make_pair(H, W, D, seed=700 + i)
        pair = mb / ("pair%d" % i)
        os.makedirs(str(pair))
        for name, img in (("im0.png", left), ("im1.png", right)):
            Image.fromarray(img, mode="L").save(str(pair / name))
        fx, fy, cx, cy, baseline, doffs = CALIBS[i]
        (pair / "calib.txt").write_text(TEXTS[0] % (fx, cx, fy, cy, doffs, baseline, W, H, D, D) if i == 0 else
                                        TEXTS[1] % (baseline, doffs, W, H, D, fx, cx, fy, cy, D))
        greys.append(np.asarray(left, np.uint8))
    (root / "mb.txt").write_text("".join("%s/im0.png\n" % (mb / ("pair%d" % i)) for i in range(2)))
    return dict(root=root, greys=greys)


@pytest.fixture(scope="module")
def runs(tree):
    root = tree["root"]
    files = {}
    for name, extra in LOOPS:
        r = _run(root / "mb.txt", root / "mb", root / ("out_" + name), 2, FLAGS + extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        files[name] = _files(root / ("out_" + name))
    r = _run(root / "mb.txt", root / "mb", root / "out_base", 2, [])
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    files["base"] = _files(root / "out_base")
    return files


def test_three_loops_write_the_same_bytes_and_the_other_files_keep_theirs(runs):
    plain = runs["plain"]
    new = sorted(f for f in plain if os.path.basename(f) in NEW)
    assert len(new) == 4, sorted(plain)
    for other in ("two", "pipe"):
        got = runs[other]
        assert sorted(got) == sorted(plain)
        for f in plain:
            assert got[f] == plain[f], "%s: %s differs from the flagless loop" % (other, f)
    base = runs["base"]
    assert sorted(base) == sorted(f for f in plain if os.path.basename(f) not in NEW)
    for f, blob in base.items():
        assert plain[f] == blob, "%s changed with --depth --point_cloud" % f


def _pfm(blob, tmp_path):
    import util
    p = tmp_path / "read.pfm"
    p.write_bytes(blob)
    return np.asarray(util.readPfm(str(p)), np.float32).reshape(H, W)


def test_files_equal_the_restatement_of_the_written_map(tree, runs, tmp_path):
    from calibration import Calibration, read_ply
    plain = runs["plain"]
    counts = []
    for i in range(2):
        rel = os.path.join("submit_v", "trainingG", "pair%d" % i)
        calib = Calibration.from_middlebury(str(tree["root"] / "mb" / "trainingG" / ("pair%d" % i) / "calib.txt"))
        assert tuple(calib) == CALIBS[i]
        disp = _pfm(plain[os.path.join(rel, "disp0MCCNN.pfm")], tmp_path)
        depth = _pfm(plain[os.path.join(rel, "depth0MCCNN.pfm")], tmp_path)
        assert np.array_equal(ref.bits(depth), ref.bits(ref.depth(disp, calib))), "pair %d: depth0MCCNN.pfm" % i
        want = ref.points(disp, calib, MAX_DEPTH)
        p = tmp_path / "read.ply"
        p.write_bytes(plain[os.path.join(rel, "points0MCCNN.ply")])
        xyz, intensity = read_ply(str(p))
        assert np.array_equal(ref.bits(xyz), ref.bits(want[:, :3])), "pair %d: points0MCCNN.ply, the device's order" % i
        pix = want[:, 3].copy().view(np.uint32)
        assert np.array_equal(intensity, tree["greys"][i].reshape(-1)[pix]), "pair %d: the intensities" % i
        counts.append(xyz.shape[0])
    assert 0 < counts[0] and 0 < counts[1], counts
    assert any(c < H * W for c in counts), "--max_depth dropped nothing: %r" % (counts,)


def test_calib_flag_overrides_the_files(tree, runs, tmp_path):
    root = tree["root"]
    text = ",".join(repr(v) for v in CALIBS[1])
    r = _run(root / "mb.txt", root / "mb", root / "out_calib", 1, ["--depth", "--calib", text])
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    got = _files(root / "out_calib")
    rel = os.path.join("submit_v", "trainingG", "pair0")
    assert not [f for f in got if f.endswith(".ply")]
    disp = _pfm(got[os.path.join(rel, "disp0MCCNN.pfm")], tmp_path)
    assert got[os.path.join(rel, "disp0MCCNN.pfm")] == runs["plain"][os.path.join(rel, "disp0MCCNN.pfm")]
    depth = _pfm(got[os.path.join(rel, "depth0MCCNN.pfm")], tmp_path)
    assert np.array_equal(ref.bits(depth), ref.bits(ref.depth(disp, CALIBS[1])))


def test_parser_errors(tree):
    root = tree["root"]
    for extra, text in ((["--depth", "--dataset", "kitti2015"], "--depth is not available with --dataset"),
                        (["--max_depth", "5"], "--max_depth goes with --point_cloud")):
        r = _run(root / "mb.txt", root / "mb", root / "out_refused", 2, extra)
        out = r.stdout.decode()
        assert r.returncode == 2 and text in out, out[-2000:]
    assert not os.path.exists(str(root / "out_refused"))
