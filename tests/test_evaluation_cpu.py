"""CPU: the evaluation's definition restated twice (tests/evaluation_reference.py: NumPy vs a per-pixel loop), the
Metrics arithmetic, the ground-truth loader, and what the built library and train.py refuse without a GPU."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import evaluation_reference as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mccnn.h")
THR = (0.5, 1.0, 2.0, 4.0)


def _tree(terms):
    x = list(terms) + [0.0] * (1024 - len(terms))
    s = 512
    while s >= 1:
        for j in range(s):
            x[j] += x[j + s]
        s //= 2
    return x[0]


@pytest.mark.parametrize("H,W,with_mask", [(1, 1, True), (3, 7, True), (5, 9, False), (16, 40, True), (31, 33, True)])
def test_restatement_equals_the_per_pixel_definition(H, W, with_mask):
    disp, gt, mask = ref.make_case(H, W, seed=H * 100 + W, with_mask=with_mask)
    got = ref.evaluate(disp, gt, mask, THR)
    loop = ref.evaluate_loop(disp, gt, mask, THR)
    assert H * W <= 1024                      # one chunk: the loop's terms through the literal tree
    for name in ref.REGIONS:
        g, w = got[name], loop[name]
        assert (g["n_valid"], g["n_invalid"], g["n_bad"]) == (w["n_valid"], w["n_invalid"], w["n_bad"])
        assert ref.bits(g["sum_abs"]) == ref.bits(0.0 + _tree(w["terms_abs"]))
        assert ref.bits(g["sum_sq"]) == ref.bits(0.0 + _tree(w["terms_sq"]))
    if mask is None:
        assert got["all"] == got["nonocc"]
    if H * W >= 16:
        assert got["all"]["n_invalid"] >= 4               # NaN, +inf, -inf and -1; -0.0 is valid
        assert got["all"]["n_valid"] <= H * W - 3         # +inf, -inf and NaN ground truth


def test_restatement_chunks_in_ascending_order():
    """Two chunks whose partials do not commute with the start value: ((0 + p0) + p1) with p0 = 1e17, p1 = tiny terms."""
    terms = np.zeros(2048)
    terms[0] = 1e17
    terms[1024:] = 1.0                       # partial 1024.0; 1e17 + 1024 rounds, 1024 x (1e17 + 1) would not move
    assert ref.tree_sum(terms) == 1e17 + 1024.0
    terms = np.arange(1500, dtype=np.float64) * 0.1
    x = list(terms[:1024])
    y = list(terms[1024:])
    assert ref.bits(ref.tree_sum(terms)) == ref.bits((0.0 + _tree(x)) + _tree(y))


def test_threshold_equality_does_not_count_and_invalid_rules():
    gt = np.array([[10.0, 10.0, 10.0, 10.0, np.inf, 10.0, 10.0]], np.float32)
    disp = np.array([[10.5, 10.5000019, -0.0, -1.0, 3.0, np.nan, np.inf]], np.float32)
    mask = np.array([[255, 255, 255, 128, 255, 255, 0]], np.uint8)
    r = ref.evaluate(disp, gt, mask, (0.5,))
    assert r["all"]["n_valid"] == 6 and r["all"]["n_invalid"] == 3 and r["all"]["n_bad"] == [2]     # 10.50000x and -0.0
    assert r["nonocc"]["n_valid"] == 4 and r["nonocc"]["n_invalid"] == 1 and r["nonocc"]["n_bad"] == [2]


def test_metrics_arithmetic_and_zero_denominators():
    import evaluation as ev
    from _hipabi import EvalResult
    res = EvalResult()
    res.all.n_valid, res.all.n_invalid = 200, 20
    res.all.n_bad[0], res.all.n_bad[1] = 50, 10
    res.all.sum_abs, res.all.sum_sq = 90.0, 720.0
    m = ev.Metrics.from_result(bytes(res), (1.0, 2.0))
    a = m.figures["all"]
    assert a["bad"] == {"1.0": 100.0 * 70 / 200, "2.0": 100.0 * 30 / 200} and a["invalid"] == 10.0
    assert a["avgerr"] == 0.5 and a["rms"] == 2.0 and m.bad(2.0, "all") == 15.0
    n = m.figures["nonocc"]           # empty region: every figure None, never NaN, never an exception
    assert n["bad"] == {"1.0": None, "2.0": None} and n["invalid"] is None and n["avgerr"] is None and n["rms"] is None
    text = json.dumps(m.to_dict())
    assert "NaN" not in text and json.loads(text)["nonocc"]["rms"] is None
    assert json.loads(text)["raw"]["all"]["sum_sq"] == 720.0
    # every pixel invalid: rates defined, errors not
    res.nonocc.n_valid = res.nonocc.n_invalid = 7
    n = ev.Metrics.from_result(bytes(res), (1.0, 2.0)).figures["nonocc"]
    assert n["bad"] == {"1.0": 100.0, "2.0": 100.0} and n["invalid"] == 100.0 and n["avgerr"] is None and n["rms"] is None
    mean = ev.mean_of([m, ev.Metrics.from_result(bytes(res), (1.0, 2.0))])
    assert mean["all"]["avgerr"] == 0.5 and mean["nonocc"]["avgerr"] is None and mean["nonocc"]["invalid"] == 100.0
    assert ev.parse_thresholds("0.5,1,2,4") == (0.5, 1.0, 2.0, 4.0)
    for bad in ("", "nan", "1,2,3,4,5,6,7,8,9"):
        with pytest.raises(ValueError):
            ev.parse_thresholds(bad)


def test_struct_mirror_is_192_bytes():
    from _hipabi import EvalRegion, EvalResult
    assert ctypes.sizeof(EvalRegion) == 96 and ctypes.sizeof(EvalResult) == 192
    assert EvalResult.nonocc.offset == 96 and EvalRegion.sum_abs.offset == 80 and EvalRegion.n_bad.offset == 16


def test_load_ground_truth(tmp_path):
    from PIL import Image
    import evaluation as ev
    import util
    rng = np.random.default_rng(1)
    gt = rng.uniform(0, 30, (9, 13)).astype(np.float32)
    gt[2, 3] = gt[8, 0] = np.inf
    mask = rng.choice(np.array([0, 128, 255], np.uint8), size=(9, 13))
    for name in ("with_mask", "without_mask", "nothing"):
        os.makedirs(str(tmp_path / name))
    for name in ("with_mask", "without_mask"):
        util.writePfm(gt, str(tmp_path / name / "disp0GT.pfm"))
    Image.fromarray(mask, mode="L").save(str(tmp_path / "with_mask" / "mask0nocc.png"))
    g, m = ev.load_ground_truth(str(tmp_path / "with_mask" / "im0.png"))
    assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), gt.view(np.uint32)) and np.isposinf(g[2, 3])
    assert m.dtype == np.uint8 and np.array_equal(m, mask)
    g, m = ev.load_ground_truth(str(tmp_path / "without_mask" / "im0.png"))
    assert m is None and np.array_equal(g.view(np.uint32), gt.view(np.uint32))
    assert ev.load_ground_truth(str(tmp_path / "nothing" / "im0.png")) is None
    with pytest.raises(ValueError, match=r"\(9, 13\).*\(9, 14\)"):
        ev.check_shape(g, (9, 14), "pair")


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"size_t\s+mccnn_evaluate_scratch_bytes\s*\(\s*int H,\s*int W\s*\)", text)
    assert re.search(r"int\s+mccnn_evaluate\s*\(\s*const float \*disp,\s*const float \*gt,\s*const uint8_t \*mask", text)
    assert "#define MCCNN_EVAL_MAX_THRESHOLDS 8" in text and "mccnn_eval_region_t all, nonocc;" in text
    assert re.search(r"#define MCCNN_ABI_VERSION 7\b", text)


def test_refusals_without_a_gpu():
    """Every refusal happens before any HIP call: its code comes back from the built library on a box without a GPU."""
    import _hipabi
    lib = _hipabi.load()
    assert lib.mccnn_evaluate_scratch_bytes(0, 5) == 0 and lib.mccnn_evaluate_scratch_bytes(5, -1) == 0
    one = lib.mccnn_evaluate_scratch_bytes(1, 1)
    assert one >= 4 * 8 + 20 * 4 and lib.mccnn_evaluate_scratch_bytes(1, 1025) >= 2 * (4 * 8 + 20 * 4)
    assert lib.mccnn_evaluate_scratch_bytes(65535, 16385) >= 65535 * 16385 // 1024 * 112
    thr = (ctypes.c_float * 8)(0.5, 1, 2, 4, 5, 6, 7, 8)
    p = ctypes.c_void_p(4096)        # never dereferenced: the call is refused first
    H, W = 4, 5
    big = ctypes.c_size_t(1 << 20)

    def call(disp=p, gt=p, mask=None, H=H, W=W, thr=thr, n=4, result=p, scratch=p, nbytes=big):
        return lib.mccnn_evaluate(disp, gt, mask, H, W, thr, n, 0, result, scratch, nbytes, None)

    for kw in (dict(disp=None), dict(gt=None), dict(thr=None), dict(result=None), dict(scratch=None)):
        assert call(**kw) == _hipabi.MCCNN_E_INVALID, kw
        assert b"null pointer" in lib.mccnn_last_error_string()
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(n=0), dict(n=9), dict(n=-1)):
        assert call(**kw) == _hipabi.MCCNN_E_INVALID, kw
    nan = (ctypes.c_float * 2)(0.5, float("nan"))
    assert call(thr=nan, n=2) == _hipabi.MCCNN_E_INVALID and b"NaN" in lib.mccnn_last_error_string()
    assert call(nbytes=ctypes.c_size_t(one - 1)) == _hipabi.MCCNN_E_SCRATCH
    assert call(nbytes=ctypes.c_size_t(0)) == _hipabi.MCCNN_E_SCRATCH
    # beyond the chunk index: 2^31 - 1 chunks of 1024 pixels; 65535 x 16385 is far inside (refused for its scratch only)
    assert call(H=2 ** 31 - 1, W=1025) == _hipabi.MCCNN_E_UNSUPPORTED
    assert call(H=65535, W=16385) == _hipabi.MCCNN_E_SCRATCH


def test_train_val_error_is_refused_without_a_gpu(tmp_path, capsys):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["--list_dir", str(tmp_path), "--tensorboard_dir", str(tmp_path / "tb"), "--checkpoint_dir",
                    str(tmp_path / "ck"), "--val_error"])
    assert e.value.code == 2 and "--val_error" in capsys.readouterr().err
    assert not (tmp_path / "tb").exists()
    with pytest.raises(SystemExit):
        train.parse_args(["--list_dir", "x", "--tensorboard_dir", "x", "--checkpoint_dir", "x", "--save_best"])
