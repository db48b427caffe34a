"""GPU: match.py --pipeline on files - the same outputs, byte for byte, as the flagless list loop (itself pinned to the
CPU checker by tests/test_cli_gpu.py), with graph replay really happening."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu


def _write_pair(dirname, H, W, ndisp, seed, rgb=False):
    from PIL import Image
    import synthetic
    os.makedirs(dirname)
    left, right, _ = synthetic.make_scene_u8(H, W, ndisp, seed=seed)
    for name, g8 in (("im0.png", left), ("im1.png", right)):
        if rgb:
            Image.fromarray(np.ascontiguousarray(np.stack([g8, 255 - g8, g8 // 3], axis=2)), mode="RGB").save(
                os.path.join(dirname, name))
        else:
            Image.fromarray(g8, mode="L").save(os.path.join(dirname, name))
    with open(os.path.join(dirname, "calib.txt"), "w") as f:
        f.write("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (W, H, ndisp, ndisp))


def test_pipeline_cli_writes_the_flagless_files_and_replays(tmp_path):
    """Seven pairs - four of 40x64x16 in a row, one 32x48x8, two 40x64x16, the last stored as RGB - through the flagless
    run, --pipeline, and --pipeline --pairs_in_flight 2: every .pfm and .pgm byte-identical to the flagless run's, every
    time file positive; with one slot the summary shows a capture and two pairs that only replayed."""
    data = tmp_path / "data"
    shapes = [(40, 64, 16)] * 4 + [(32, 48, 8)] + [(40, 64, 16)] * 2
    rels = ["s/p%d" % i for i in range(len(shapes))]
    for i, (rel, (H, W, D)) in enumerate(zip(rels, shapes)):
        _write_pair(str(data / rel), H, W, D, seed=80 + i, rgb=(i == len(shapes) - 1))
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in rels))
    script = os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py")
    common = [sys.executable, script, "--list_file", str(lst), "--resume", os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"),
              "--data_dir", str(data), "-s", "0", "-e", str(len(rels) - 1), "-t", "r"]
    logs = {}
    for name, extra in (("plain", []), ("pipe", ["--pipeline"]), ("pipe2", ["--pipeline", "--pairs_in_flight", "2"])):
        r = subprocess.run(common + ["--save_dir", str(tmp_path / name)] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=900)
        logs[name] = r.stdout.decode()
        assert r.returncode == 0, logs[name][-3000:]
    assert "pipeline:" not in logs["plain"]
    for name in ("pipe", "pipe2"):
        for rel, (H, W, _) in zip(rels, shapes):
            for root, fn in (("submit_r", "disp0MCCNN.pfm"), ("submit_r_imgs", "disp0MCCNN.pgm")):
                a = (tmp_path / "plain" / root / rel / fn).read_bytes()
                b = (tmp_path / name / root / rel / fn).read_bytes()
                assert a == b and len(a) > H * W, (name, rel, fn)
            assert float((tmp_path / name / "submit_r" / rel / "timeMCCNN.txt").read_text()) > 0
        m = re.findall(r"pipeline: pairs=(\d+) captures=(\d+) replays=(\d+) eager=(\d+)", logs[name])
        assert len(m) == 1, logs[name][-2000:]
        pairs, captures, replays, eager = map(int, m[0])
        assert pairs == 7 and captures + replays + eager == 7
        if name == "pipe":
            assert captures >= 1 and replays >= 2, m


def test_pipeline_cli_refuses_a_shape_outside_the_envelope(tmp_path):
    """ndisp beyond the image's width: today's message, a non-zero exit, and the pair before it is still written."""
    data = tmp_path / "data"
    _write_pair(str(data / "a"), 32, 48, 8, seed=1)
    _write_pair(str(data / "b"), 32, 48, 8, seed=2)
    calib = data / "b" / "calib.txt"
    calib.write_text(calib.read_text().replace("ndisp=8", "ndisp=47"))
    lst = tmp_path / "list.txt"
    lst.write_text("%s/im0.png\n%s/im0.png\n" % (data / "a", data / "b"))
    script = os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py")
    r = subprocess.run([sys.executable, script, "--list_file", str(lst), "--resume",
                        os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"), "--data_dir", str(data), "--save_dir",
                        str(tmp_path / "out"), "-s", "0", "-e", "1", "-t", "r", "--pipeline"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    log = r.stdout.decode()
    assert r.returncode != 0
    assert "ndisp=47 needs an image at least ndisp + 2 = 49 pixels wide, got W=48" in log, log[-2000:]
    assert (tmp_path / "out" / "submit_r" / "a" / "disp0MCCNN.pfm").is_file()
    assert not (tmp_path / "out" / "submit_r" / "b").exists()
