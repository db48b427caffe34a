"""GPU: match.py --arch accurate end to end on files - the outputs are written, --pipeline writes the same bytes, and a
run without the flag writes what the fast network's matcher returns, as before."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from test_cli_gpu import _write_pair

pytestmark = pytest.mark.gpu

H, W, D = 40, 64, 16
RELS = ["trainingH/pairA", "trainingH/pairB"]
OUTPUTS = ("disp0MCCNN.pfm",)


def _run(tmp_path, tag, extra):
    data, out = tmp_path / "data", tmp_path / "out"
    lst = tmp_path / "list.txt"
    if not data.exists():
        for i, rel in enumerate(RELS):
            _write_pair(str(data / rel), H, W, D, seed=40 + i)
        lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in RELS))
    cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0", "--list_file", str(lst),
           "--data_dir", str(data), "--save_dir", str(out), "-t", tag, "-s", "0", "-e", "1"] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    files = {}
    for rel in RELS:
        res = out / ("submit_%s" % tag) / rel
        img = out / ("submit_%s_imgs" % tag) / rel
        assert (res / "timeMCCNN.txt").is_file() and float((res / "timeMCCNN.txt").read_text().strip()) > 0.0
        files[rel] = ((res / "disp0MCCNN.pfm").read_bytes(), (img / "disp0MCCNN.pgm").read_bytes())
    return data, files


def _standardised(path):
    import util
    g = util.read_gray(str(path)).astype(np.float32)
    return np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2)


def _pfm(blob, tmp_path):
    import util
    p = tmp_path / "read.pfm"
    p.write_bytes(blob)
    disp = util.readPfm(str(p))
    disp = disp[0] if isinstance(disp, tuple) else disp
    return np.asarray(disp, np.float32).reshape(H, W)


def test_match_cli_accurate(tmp_path):
    import torch
    import helpers
    import stereo_device as sd
    from model import ACCURATE_NET
    ckpt = str(tmp_path / "accurate.npz")
    ACCURATE_NET(None, device="cpu", seed=21).save(ckpt)
    data, plain = _run(tmp_path, "acc", ["--arch", "accurate", "--resume", ckpt])
    _data, piped = _run(tmp_path, "accp", ["--arch", "accurate", "--resume", ckpt, "--pipeline"])
    for rel in RELS:
        assert plain[rel][0] == piped[rel][0], "%s: --pipeline wrote another disp0MCCNN.pfm" % rel
        assert plain[rel][1] == piped[rel][1], "%s: --pipeline wrote another disp0MCCNN.pgm" % rel
    # the files hold what the matcher returns for the same decoded pair
    net = ACCURATE_NET(None, batch_size=1, device="cuda").restore(ckpt)
    m = sd.StereoMatcher(net)
    for rel in RELS:
        L, R = (_standardised(data / rel / n) for n in ("im0.png", "im1.png"))
        want = m.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), D).cpu().numpy()
        helpers.assert_bits_strict(_pfm(plain[rel][0], tmp_path), want, "%s: --arch accurate" % rel)
    assert plain[RELS[0]][0] != plain[RELS[1]][0]


def test_match_cli_without_arch_is_the_fast_network(tmp_path, net_layers):
    import torch
    import helpers
    import stereo_device as sd
    from model import NET
    fast = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
    data, files = _run(tmp_path, "fast", ["--resume", fast])
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    m = sd.StereoMatcher(net)
    for rel in RELS:
        L, R = (_standardised(data / rel / n) for n in ("im0.png", "im1.png"))
        want = m.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), D).cpu().numpy()
        helpers.assert_bits_strict(_pfm(files[rel][0], tmp_path), want, "%s: default command line" % rel)
