"""CPU: the host side of the KITTI support - the data set layouts' path mapping, the 16-bit PNG round trip, the float
convention, the restated background interpolation (the kit's sequential walks say what the nearest-valid definition of
include/mccnn.h says), the argument validation of the new entry points, the abs[:rel] parser and match.py's refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kitti_reference as kr
from conftest import GOLDEN_DIR, ROOT

SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")


# ---- layouts ----------------------------------------------------------------------------------------------------------
def test_kitti2015_paths():
    import datasets
    k = datasets.get("kitti2015")
    left = "/data/kitti/training/image_2/000007_10.png"
    assert k.right(left) == "/data/kitti/training/image_3/000007_10.png"
    assert k.truth_paths(left) == ("/data/kitti/training/disp_occ_0/000007_10.png",
                                   "/data/kitti/training/disp_noc_0/000007_10.png")
    out = k.outputs(left, "/data/kitti", "/out/submit_t", "/out/submit_t_imgs")
    assert out["out"] == "/out/submit_t/disp_0/000007_10.png"
    assert out["out_time"] == "/out/submit_t/time/000007_10.txt"
    assert out["out_eval"] == "/out/submit_t/eval/000007_10.json"
    assert out["out_img"] == "/out/submit_t_imgs/training/image_2/000007_10.pgm"
    assert set(os.path.dirname(out[key]) for key in ("out", "out_time", "out_eval", "out_img")) == set(out["dirs"])
    with pytest.raises(ValueError, match="image_2"):
        k.right("/data/kitti/training/colored_0/000007_10.png")


def test_kitti2012_takes_the_colour_or_the_grey_views():
    import datasets
    k = datasets.get("kitti2012")
    assert k.right("/d/training/colored_0/000001_10.png") == "/d/training/colored_1/000001_10.png"
    assert k.right("/d/training/image_0/000001_10.png") == "/d/training/image_1/000001_10.png"
    for view in ("colored_0", "image_0"):
        left = "/d/training/%s/000001_10.png" % view
        assert k.truth_paths(left) == ("/d/training/disp_occ/000001_10.png", "/d/training/disp_noc/000001_10.png")
        assert k.outputs(left, "/d", "/o/submit_t", "/o/submit_t_imgs")["out"] == "/o/submit_t/000001_10.png"
    with pytest.raises(ValueError, match="colored_0 or image_0"):
        k.right("/d/training/image_2/000001_10.png")


def test_middlebury_layout_is_the_suffix_replacement():
    import datasets
    import match
    m = datasets.get("middlebury")
    left = "/data/mb/trainingH/Adirondack/im0.png"
    assert m.right(left) == left.replace(match.left_image_suffix, match.right_image_suffix)
    assert m.calib(left) == left.replace(match.left_image_suffix, match.calib_suffix)
    assert m.truth_paths(left) == (left.replace(match.left_image_suffix, match.left_gt_suffix),)
    out = m.outputs(left, "/data/mb", "/o/submit_t", "/o/submit_t_imgs")
    assert out["out"] == "/o/submit_t/trainingH/Adirondack/disp0MCCNN.pfm"
    assert out["out_time"] == "/o/submit_t/trainingH/Adirondack/timeMCCNN.txt"
    assert out["out_img"] == "/o/submit_t_imgs/trainingH/Adirondack/disp0MCCNN.pgm"
    assert out["out_eval"] == "/o/submit_t/trainingH/Adirondack/evalMCCNN.json"
    assert not m.kitti and datasets.get("kitti2012").kitti and datasets.get("kitti2015").kitti


def test_shape_comes_from_the_left_image_and_the_flag(tmp_path):
    from PIL import Image
    import datasets
    os.makedirs(str(tmp_path / "image_2"))
    left = str(tmp_path / "image_2" / "000000_10.png")
    Image.fromarray(np.zeros((38, 62, 3), np.uint8)).save(left)
    k = datasets.get("kitti2015")
    assert k.shape(left) == (38, 62, 228) and k.shape(left, 16) == (38, 62, 16)
    assert k.shape(left, 16, np.zeros((40, 64), np.uint8)) == (40, 64, 16)


# ---- files ------------------------------------------------------------------------------------------------------------
def test_png_u16_round_trip(tmp_path):
    import util
    code = np.random.default_rng(0).integers(0, 65536, (37, 61)).astype(np.uint16)
    code[0, :4] = (0, 1, 255, 65535)
    path = str(tmp_path / "a.png")
    util.write_png_u16(code, path)
    back = util.read_u16(path)
    assert back.dtype == np.uint16 and back.flags["C_CONTIGUOUS"] and np.array_equal(back, code)
    from PIL import Image
    assert Image.open(path).mode == "I;16"
    Image.fromarray(np.zeros((4, 4), np.uint8)).save(str(tmp_path / "b.png"))
    with pytest.raises(ValueError, match="16-bit"):
        util.read_u16(str(tmp_path / "b.png"))


def test_kitti_gt_to_float():
    import datasets
    code = np.array([[0, 1, 256, 384, 65535]], np.uint16)
    got = datasets.kitti_gt_to_float(code)
    assert got.dtype == np.float32 and np.isposinf(got[0, 0])
    assert got[0, 1:].tolist() == [1 / 256, 1.0, 1.5, 65535 / 256]
    assert np.array_equal(kr.u32(got), kr.u32(kr.decode(code)))
    with pytest.raises(ValueError):
        datasets.kitti_gt_to_float(code.astype(np.int32))
    # encode is the inverse on every code but "no value", and a valid zero does not read back as one
    assert np.array_equal(kr.encode(got[:, 1:]), code[:, 1:])
    assert kr.encode(np.zeros((1, 1), np.float32))[0, 0] == 1 and kr.encode(np.full((1, 1), np.inf, np.float32))[0, 0] == 0


def test_encode_restatement_on_the_named_values():
    for value, code in kr.encode_specials():
        assert kr.encode(np.array([[value]], np.float32))[0, 0] == code, (value, code)


# ---- the parallel definition says what the kit's loops do ------------------------------------------------------------
@pytest.mark.parametrize("H,W,seed", [(1, 1, 0), (1, 7, 1), (2, 64, 2), (3, 65, 3), (5, 130, 4), (4, 257, 5), (9, 33, 6)])
def test_literal_walks_equal_the_nearest_valid_formulation(H, W, seed):
    rng = np.random.default_rng(seed)
    for trial in range(6):
        whole = tuple(int(r) for r in np.flatnonzero(rng.random(H) < (0.3 if trial % 2 else 0.0)))
        m = kr.make_holes_map(H, W, seed=100 * seed + trial, whole_rows=whole)
        if trial == 5:
            m = np.where(rng.random((H, W)) < 0.9, np.float32(np.nan), m).astype(np.float32)      # mostly holes
        walk, near = kr.interpolate_background_walk(m), kr.interpolate_background_nearest(m)
        assert np.array_equal(kr.u32(walk), kr.u32(near)), (H, W, trial)
        ok = kr.valid(m)
        assert np.array_equal(kr.u32(walk[ok]), kr.u32(m[ok]))                       # valid pixels bit for bit
        assert np.array_equal(kr.valid(walk).all(axis=1) | ~kr.valid(walk).any(axis=1), np.ones(H, bool))
    empty = np.full((H, W), -1.0, np.float32)
    assert np.array_equal(kr.u32(kr.interpolate_background_walk(empty)), kr.u32(empty))


def test_walk_on_a_hand_made_map():
    n = np.nan
    m = np.array([[n, n, n, n, n],
                  [n, 3, n, 1, n],
                  [n, n, n, n, n],
                  [2, n, n, 5, 4],
                  [n, n, n, n, n]], np.float32)
    want = np.array([[3, 3, 1, 1, 1],
                     [3, 3, 1, 1, 1],
                     [n, n, n, n, n],
                     [2, 2, 2, 5, 4],
                     [2, 2, 2, 5, 4]], np.float32)
    for f in (kr.interpolate_background_walk, kr.interpolate_background_nearest):
        assert np.array_equal(kr.u32(f(m)), kr.u32(want))


# ---- argument validation without a GPU --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import _hipabi
    if not os.path.isfile(_hipabi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mc-cnn-python_amd"), "-j4"])
    return _hipabi.load()


def _buf(nbytes, offset=0):
    """A host address with the asked alignment: validation happens before any HIP call, nothing is dereferenced."""
    raw = ctypes.create_string_buffer(nbytes + 64)
    base = (ctypes.addressof(raw) + 63) & ~63
    return raw, ctypes.c_void_p(base + offset)


def test_encode_and_interpolate_validate_their_arguments(lib):
    keep, a = _buf(64)
    keep2, b = _buf(64)
    _k3, odd = _buf(64, 1)
    _k4, two = _buf(64, 2)
    err = lib.mccnn_last_error_string
    assert lib.mccnn_kitti_encode_u16(None, 2, 2, b, None) == -1 and b"mccnn_kitti_encode_u16: null pointer" in err()
    assert lib.mccnn_kitti_encode_u16(a, 2, 2, None, None) == -1 and b"null pointer" in err()
    assert lib.mccnn_kitti_encode_u16(a, 0, 2, b, None) == -1 and b"non-positive size" in err()
    assert lib.mccnn_kitti_encode_u16(a, 2, -1, b, None) == -1 and b"non-positive size" in err()
    assert lib.mccnn_kitti_encode_u16(a, 2, 2, odd, None) == -1 and b"aligned" in err()
    assert lib.mccnn_kitti_encode_u16(two, 2, 2, b, None) == -1 and b"aligned" in err()
    assert lib.mccnn_kitti_encode_u16(a, 2 ** 31 - 1, 2 ** 31 - 1, b, None) == -2 and b"H*W" in err()
    f = lib.mccnn_kitti_decode_u16
    assert f(None, 2, 2, b, None) == -1 and b"mccnn_kitti_decode_u16: null pointer" in err()
    assert f(a, 2, 2, None, None) == -1 and b"null pointer" in err()
    assert f(a, -2, 2, b, None) == -1 and b"non-positive size" in err()
    assert f(odd, 2, 2, b, None) == -1 and b"aligned" in err()
    assert f(a, 2, 2, two, None) == -1 and b"aligned" in err()
    assert f(a, 2 ** 31 - 1, 2 ** 31 - 1, b, None) == -2 and b"H*W" in err()
    f = lib.mccnn_kitti_interpolate_background
    assert f(None, 2, 2, b, None) == -1 and b"mccnn_kitti_interpolate_background: null pointer" in err()
    assert f(a, 2, 2, None, None) == -1 and b"null pointer" in err()
    assert f(a, 2, 0, b, None) == -1 and b"non-positive size" in err()
    assert f(a, 2, 2, a, None) == -1 and b"out must not be disp" in err()
    assert f(a, 2, 2, two, None) == -1 and b"aligned" in err()


def test_evaluate_kitti_validates_its_arguments(lib):
    floats = ctypes.c_float * 8
    abs_thr, rel_thr = floats(3, 1, 2, 3, 4, 5, 6, 7), floats(0.05, 0, 0, 0, 0, 0, 0, 0)
    _k = [_buf(4096) for _ in range(4)]
    d, g, res, scr = (p for _, p in _k)
    _k5, odd = _buf(64, 1)
    _k6, four = _buf(4096, 4)
    err = lib.mccnn_last_error_string
    f = lib.mccnn_evaluate_kitti
    H, W = 4, 5
    need = lib.mccnn_evaluate_kitti_scratch_bytes(H, W, 0)
    need_i = lib.mccnn_evaluate_kitti_scratch_bytes(H, W, 1)
    assert need == lib.mccnn_evaluate_scratch_bytes(H, W) and need_i >= need + H * W * 4 and need_i % 8 == 0
    assert lib.mccnn_evaluate_kitti_scratch_bytes(0, 5, 1) == 0 and lib.mccnn_evaluate_kitti_scratch_bytes(5, -1, 0) == 0

    def call(disp=d, occ=g, noc=None, h=H, w=W, a=abs_thr, r=rel_thr, n=1, interp=0, result=res, scratch=scr, nbytes=4096):
        return f(disp, occ, noc, h, w, a, r, n, interp, 0, result, scratch, nbytes, None)

    for kw in (dict(disp=None), dict(occ=None), dict(a=None), dict(r=None), dict(result=None), dict(scratch=None)):
        assert call(**kw) == -1 and b"mccnn_evaluate_kitti: null pointer" in err(), kw
    assert call(h=0) == -1 and b"non-positive size" in err()
    assert call(w=-3) == -1 and b"non-positive size" in err()
    assert call(n=0) == -1 and b"n_thr=0, expected 1..8" in err()
    assert call(n=9) == -1 and b"n_thr=9" in err()
    assert call(a=floats(float("nan"))) == -1 and b"threshold 0 is NaN" in err()
    assert call(r=floats(0, float("nan")), n=2) == -1 and b"threshold 1 is NaN" in err()
    assert call(a=floats(-1.0)) == -1 and b"threshold 0 is negative" in err()
    assert call(r=floats(-0.05)) == -1 and b"threshold 0 is negative" in err()
    assert call(nbytes=need - 1) == -3 and b"mccnn_evaluate_kitti_scratch_bytes(4, 5, 0)" in err()
    assert call(interp=1, nbytes=need_i - 1) == -3 and b"mccnn_evaluate_kitti_scratch_bytes(4, 5, 1)" in err()
    assert call(scratch=four) == -1 and b"8-byte aligned" in err()
    assert call(result=four) == -1 and b"8-byte aligned" in err()
    assert call(occ=odd) == -1 and b"2-byte aligned" in err()
    assert call(noc=odd) == -1 and b"2-byte aligned" in err()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1, nbytes=2 ** 62) == -2 and b"H*W" in err()


# ---- command lines ----------------------------------------------------------------------------------------------------
def test_abs_rel_parser():
    import evaluation as ev
    assert ev.parse_kitti_thresholds("3:0.05") == ((3.0, 0.05),)
    assert ev.parse_kitti_thresholds("2,3,4,5") == ((2.0, 0.0), (3.0, 0.0), (4.0, 0.0), (5.0, 0.0))
    assert ev.parse_kitti_thresholds(" 3:0.05, 2 ,") == ((3.0, 0.05), (2.0, 0.0))
    for bad in ("", "1,2,3,4,5,6,7,8,9", "3:0.05:1", "nan", "3:nan", "-1", "3:-0.05", "3:0.05,3", "x"):
        with pytest.raises(ValueError):
            ev.parse_kitti_thresholds(bad)
    import datasets
    assert datasets.get("kitti2015").parse_thresholds(datasets.get("kitti2015").default_thresholds) == ((3.0, 0.05),)
    assert [a for a, _ in datasets.get("kitti2012").parse_thresholds(datasets.get("kitti2012").default_thresholds)] \
        == [2.0, 3.0, 4.0, 5.0]
    assert datasets.get("middlebury").parse_thresholds(datasets.get("middlebury").default_thresholds) == ev.DEFAULT_THRESHOLDS


def _match(tmp_path, extra):
    cmd = [sys.executable, os.path.join(SRC, "match.py"), "-g", "0", "--list_file", str(tmp_path / "list.txt"), "--resume",
           os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"), "--data_dir", str(tmp_path), "--save_dir", str(tmp_path / "o"),
           "-t", "k", "-s", "0", "-e", "0"] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return r.returncode, r.stdout.decode()


def test_match_refuses_ndisp_with_middlebury_and_an_ndisp_the_frame_cannot_hold(tmp_path):
    from PIL import Image
    for view in ("image_2", "image_3"):
        os.makedirs(str(tmp_path / "training" / view))
        Image.fromarray(np.zeros((38, 62), np.uint8)).save(str(tmp_path / "training" / view / "000000_10.png"))
    (tmp_path / "list.txt").write_text("%s\n" % (tmp_path / "training" / "image_2" / "000000_10.png"))
    code, text = _match(tmp_path, ["--ndisp", "16"])
    assert code == 2 and "--ndisp goes with a KITTI --dataset" in text, text[-1500:]
    code, text = _match(tmp_path, ["--dataset", "middlebury", "--eval_interpolate"])
    assert code == 2 and "--eval_interpolate goes with a KITTI --dataset" in text, text[-1500:]
    code, text = _match(tmp_path, ["--dataset", "kitti2015", "--ndisp", "0"])
    assert code == 2 and "--ndisp must be positive" in text, text[-1500:]
    code, text = _match(tmp_path, ["--dataset", "kitti2015", "--eval_thresholds", "3:0.05,3:0.1"])
    assert code == 2 and "--eval_thresholds" in text, text[-1500:]
    # 62 pixels hold at most 60 disparities; the default 228 does not fit either.  Refused before the GPU is asked for.
    for extra, ndisp in ((["--ndisp", "61"], 61), ([], 228)):
        code, text = _match(tmp_path, ["--dataset", "kitti2015"] + extra)
        assert code != 0 and "ndisp=%d needs an image at least ndisp + 2 = %d pixels wide, got W=62" % (ndisp, ndisp + 2) in text, \
            text[-1500:]
        assert "no HIP device" not in text


def test_train_refuses_ndisp_with_middlebury():
    import train
    with pytest.raises(SystemExit):
        train.parse_args(["--list_dir", "l", "--tensorboard_dir", "t", "--checkpoint_dir", "c", "--ndisp", "16"])
    args = train.parse_args(["--list_dir", "l", "--tensorboard_dir", "t", "--checkpoint_dir", "c", "--dataset", "kitti2015"])
    assert args.ndisp == 228
    args = train.parse_args(["--list_dir", "l", "--tensorboard_dir", "t", "--checkpoint_dir", "c"])
    assert args.ndisp is None and args.dataset == "middlebury"


def test_generators_take_the_layouts_paths_and_truth(tmp_path):
    """ImageDataGenerator and the device sampler's host side (device=None) on a kitti2015 tree: sparse uint16 truth read as
    float32 with +inf, and the pool of every pixel with known disparity."""
    from PIL import Image
    import datagenerator
    import datasets
    import util
    rng = np.random.default_rng(0)
    H, W = 20, 30
    lefts = []
    for k in range(2):
        for view in ("image_2", "image_3"):
            os.makedirs(str(tmp_path / "training" / view), exist_ok=True)
            Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(
                str(tmp_path / "training" / view / ("%06d_10.png" % k)))
        cols = np.arange(W)[None, :]
        noc = (rng.integers(0, 8 * 256, (H, W)) * (rng.random((H, W)) < 0.3)).astype(np.uint16)
        noc[(noc // 256) > cols] = 0                      # the match of a known pixel lies inside the image
        occ = noc.copy()
        occ[0, 10] = 3 * 256
        for name, plane in (("disp_noc_0", noc), ("disp_occ_0", occ)):
            os.makedirs(str(tmp_path / "training" / name), exist_ok=True)
            util.write_png_u16(plane, str(tmp_path / "training" / name / ("%06d_10.png" % k)))
        lefts.append((str(tmp_path / "training" / "image_2" / ("%06d_10.png" % k)), noc))
    lst = tmp_path / "train.txt"
    lst.write_text("".join("%s\n" % p for p, _ in lefts))
    layout = datasets.get("kitti2015")
    gen = datagenerator.ImageDataGenerator(str(lst), rng=np.random.default_rng(1), layout=layout)
    assert gen.right_paths[0].endswith("training/image_3/000000_10.png") and gen.gt_paths[0].endswith("disp_noc_0/000000_10.png")
    for (_, noc), gt in zip(lefts, gen.gt_images):
        assert gt.dtype == np.float32 and np.array_equal(kr.u32(gt), kr.u32(datasets.kitti_gt_to_float(noc)))
    left, pos, neg = gen.next_batch(8)
    assert left.shape == pos.shape == neg.shape == (8, 11, 11, 1)
    pool = datagenerator.DevicePatchSampler(str(lst), rng=np.random.default_rng(1), device=None, sampling="pool",
                                            batch_size=8, layout=layout)
    assert pool.n_valid == sum(int(np.count_nonzero(noc)) for _, noc in lefts) > 0
    assert len(pool.draw(8)) == 24
