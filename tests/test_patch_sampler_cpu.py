"""CPU: the host side of the device patch sampler - the NumPy restatement of mccnn_sample_patches against
ImageDataGenerator._cut, DevicePatchSampler's drawing (pair mode replays ImageDataGenerator's random stream, pool mode
permutes every valid pixel, the augmentation draws stay in their intervals), the entry point's refusals without a GPU,
train.py's new flags and Trainer.step_stacked."""
import ctypes
import os

import numpy as np
import pytest
import torch

import patch_sampler_reference as ref


def _write_dataset(root, n_pairs=3, H=40, W=72, seed=0):
    """tests/test_train_cpu.py's builder: random-texture left views, right views shifted by a piecewise-constant
    integer disparity, ground truth with a band of unknown (inf) pixels; lists train.txt / val.txt."""
    from PIL import Image
    import util
    rng = np.random.default_rng(seed)
    lefts = []
    for i in range(n_pairs):
        d = os.path.join(root, "pair%d" % i)
        os.makedirs(d)
        scene = rng.integers(0, 256, size=(H, W + 32)).astype(np.uint8)
        gt = np.full((H, W), 4.0, np.float32)
        gt[H // 2:] = 9.0
        left = scene[:, 16:16 + W]
        right = np.zeros_like(left)
        for y in range(H):
            s = int(gt[y, 0])
            right[y] = scene[y, 16 + s:16 + s + W]              # right[y, x - s] = left[y, x]
        gt[:, :3] = np.inf                                       # unknown band: never sampled
        Image.fromarray(left, "L").save(os.path.join(d, "im0.png"))
        Image.fromarray(right, "L").save(os.path.join(d, "im1.png"))
        util.writePfm(gt, os.path.join(d, "disp0GT.pfm"))
        lefts.append(os.path.join(d, "im0.png"))
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    open(os.path.join(lists, "train.txt"), "w").write("\n".join(lefts[:-1]) + "\n")
    open(os.path.join(lists, "val.txt"), "w").write(lefts[-1] + "\n")
    return lists


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _identity_records(image, centres):
    from datagenerator import SAMPLE_DTYPE
    rec = np.zeros(len(centres), dtype=SAMPLE_DTYPE)
    rec["image"] = image
    rec["cy"], rec["cx"] = [c[0] for c in centres], [c[1] for c in centres]
    rec["m"], rec["gain"] = (1, 0, 0, 1), 1
    return rec


def test_restatement_on_identity_records_is_cut():
    """Identity records give the bits of ImageDataGenerator._cut: corners, borders and -0.0 pixels."""
    from datagenerator import ImageDataGenerator
    H, W, ps = 12, 9, 11
    img = np.random.default_rng(0).standard_normal((H, W)).astype(np.float32)
    img[0, 0] = img[H - 1, W - 1] = img[5, 4] = img[6, 2] = -0.0
    centres = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (5, 4)]
    g = ImageDataGenerator.__new__(ImageDataGenerator)
    g.patch_size = (ps, ps)
    rows, cols = (np.array([c[k] for c in centres], dtype=np.int64) for k in (0, 1))
    want = g._cut(g._padded(img), rows, cols)[..., 0]
    assert np.signbit(want).any() and (want == 0).any()              # the -0.0 pixels and the zero padding are in view
    rec = _identity_records(0, centres)
    assert np.array_equal(_bits(ref.sample_patches([img], rec, ps)), _bits(want))
    assert np.array_equal(_bits(ref.sample_patches_arrays([img], rec, ps)), _bits(want))


@pytest.mark.parametrize("ps", [1, 3, 9, 11, 13, 31])
def test_array_restatement_is_the_per_pixel_one(ps):
    """The GPU tests compare large cases with sample_patches_arrays: it is the per-pixel restatement, bit for bit, on
    records of every kind (mixed_records) and on far centres, which read nothing."""
    shapes = [(5, 7), (12, 9), (40, 72)]
    images = ref.planted_images(shapes, seed=1)
    rec = ref.mixed_records(shapes, 14 if ps < 31 else 7, ps, seed=ps)
    a, b = ref.sample_patches(images, rec, ps), ref.sample_patches_arrays(images, rec, ps)
    assert np.array_equal(_bits(a), _bits(b))
    far = (np.abs(rec["cy"]) > 1e29) | (np.abs(rec["cx"]) > 1e29)
    plain = far & (rec["bias"] == 0)
    assert not a[plain].any()


def test_pair_mode_draws_image_data_generators_centres(tmp_path):
    from datagenerator import DevicePatchSampler, ImageDataGenerator, draw_pair_centres
    lists = _write_dataset(str(tmp_path), seed=5)
    train = os.path.join(lists, "train.txt")
    for shuffle in (False, True):
        g = ImageDataGenerator(train, shuffle=shuffle, rng=np.random.default_rng(11))
        s = DevicePatchSampler(train, shuffle=shuffle, rng=np.random.default_rng(11), device=None, sampling="pair")
        twin = np.random.default_rng(11)                 # replays the shared helper beside the two classes
        order = twin.permutation(2) if shuffle else np.arange(2)
        for step in range(2):
            B = 32
            left, pos, neg = g.next_batch(B)
            rec = s.draw(B)
            assert rec.shape == (3 * B,) and s.last_records is rec
            p = int(order[step])
            rows, cols, pos_col, neg_col = draw_pair_centres(twin, s.gt_images[p], B, 0.5, 1.5, 6)
            assert np.array_equal(rec["image"], np.repeat([2 * p, 2 * p + 1, 2 * p + 1], B))
            assert np.array_equal(rec["cy"], np.tile(rows, 3).astype(np.float32))
            assert np.array_equal(rec["cx"], np.concatenate([cols, pos_col, neg_col]).astype(np.float32))
            assert (rec["m"] == (1, 0, 0, 1)).all() and (rec["gain"] == 1).all() and (rec["bias"] == 0).all()
            # ... and those records, cut by the restatement, are ImageDataGenerator's patches
            images = [im for pair in zip(s.left_images, s.right_images) for im in pair]
            got = ref.sample_patches_arrays(images, rec, 11)
            want = np.concatenate([left, pos, neg])[..., 0]
            assert np.array_equal(_bits(got), _bits(want))
        # the two generators have consumed the same random numbers
        assert g.rng.integers(0, 1 << 30) == s.rng.integers(0, 1 << 30)


def test_pool_mode_permutes_every_valid_pixel(tmp_path):
    from datagenerator import DevicePatchSampler
    lists = _write_dataset(str(tmp_path), seed=6)
    B = 50
    s = DevicePatchSampler(os.path.join(lists, "train.txt"), rng=np.random.default_rng(2), device=None, sampling="pool",
                           batch_size=B)
    n_valid = 0
    for gt in s.gt_images:
        for r in range(gt.shape[0]):
            for c in range(gt.shape[1]):
                n_valid += bool(np.isfinite(gt[r, c]) and int(gt[r, c]) <= c)
    assert s.n_valid == n_valid and s.steps_per_epoch == n_valid // B and n_valid % B != 0
    assert DevicePatchSampler(os.path.join(lists, "train.txt"), device=None, sampling="pool", batch_size=B,
                              world_size=2).steps_per_epoch == n_valid // B // 2

    def epoch():
        seen = []
        for _ in range(s.steps_per_epoch):
            rec = s.draw(B)
            assert len(rec) == 3 * B
            left, pos, neg = rec[:B], rec[B:2 * B], rec[2 * B:]
            assert (left["image"] % 2 == 0).all() and np.array_equal(pos["image"], left["image"] + 1)
            assert np.array_equal(neg["image"], pos["image"]) and np.array_equal(pos["cy"], left["cy"])
            for k in range(B):
                p, r, c = int(left["image"][k]) // 2, int(left["cy"][k]), int(left["cx"][k])
                g = s.gt_images[p][r, c]
                assert np.isfinite(g) and int(g) <= c
                W = s.gt_images[p].shape[1]
                assert 0 <= pos["cx"][k] < W and 0 <= neg["cx"][k] < W
                assert pos["cx"][k] - (c - int(g)) in (-1, 0)            # int(right_col + U(-0.5, 0.5))
                assert 1 <= abs(neg["cx"][k] - (c - int(g))) <= 6
                seen.append((p, r, c))
        return seen

    first = epoch()
    assert len(set(first)) == len(first) == s.steps_per_epoch * B
    with pytest.raises(IndexError):
        s.draw(B)                                                    # the remainder is dropped
    s.reset_pointer()
    second = epoch()
    assert len(set(second)) == len(second) and second != first


def test_subpixel_centres_keep_the_fraction(tmp_path):
    from datagenerator import DevicePatchSampler
    lists = _write_dataset(str(tmp_path), seed=7)
    for sampling in ("pair", "pool"):
        s = DevicePatchSampler(os.path.join(lists, "train.txt"), rng=np.random.default_rng(3), device=None,
                               sampling=sampling, truncate=False, batch_size=32)
        rec = s.draw(32)
        left, pos, neg = rec[:32], rec[32:64], rec[64:]
        W = 72
        for k in range(32):
            g = s.gt_images[int(left["image"][k]) // 2][int(left["cy"][k]), int(left["cx"][k])]
            true = left["cx"][k] - g
            assert abs(pos["cx"][k] - true) <= 0.5 + 1e-4 and 1.5 - 1e-4 <= abs(neg["cx"][k] - true) <= 6 + 1e-4
            assert 0 <= pos["cx"][k] <= W - 1 and 0 <= neg["cx"][k] <= W - 1
        assert (pos["cx"] != np.round(pos["cx"])).any()


def _fractional_ground_truth(lists):
    """Rewrites the list's ground truth with fractional disparities: 4.7 above, 9.3 below.  Column 4 of the upper half
    and column 9 of the lower half are pixels with int(gt) <= col < gt: valid by the reference's rule, their true match
    at col - gt = -0.7 / -0.3, left of the image."""
    import util
    for line in open(os.path.join(lists, "train.txt")):
        path = line.strip().replace("im0.png", "disp0GT.pfm")
        gt = np.asarray(util.readPfm(path), dtype=np.float32).copy()
        gt[gt == 4.0] = 4.7
        gt[gt == 9.0] = 9.3
        util.writePfm(gt, path)


def _returns(fn, seconds=30):
    """fn() on a thread of its own: a redraw loop that cannot end fails the test instead of hanging the suite."""
    import threading
    box = []
    t = threading.Thread(target=lambda: box.append(fn()), daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "the draw did not return within %d s" % seconds
    return box[0]


@pytest.mark.parametrize("sampling", ["pair", "pool"])
def test_subpixel_centres_on_fractional_ground_truth(tmp_path, sampling):
    """With the fraction kept, a pixel whose match lies left of the image (col - gt in (-1, 0)) is not a centre: from
    col - gt <= -0.5 no positive column col - gt + U(-0.5, 0.5) is inside the image, and the redraw would never end.
    The truncating rule keeps such pixels, as the reference does (int(-0.3) = 0)."""
    from datagenerator import DevicePatchSampler, draw_pair_centres
    lists = _write_dataset(str(tmp_path), seed=7)
    _fractional_ground_truth(lists)
    train = os.path.join(lists, "train.txt")
    B, W = 32, 72
    s = DevicePatchSampler(train, rng=np.random.default_rng(3), device=None, sampling=sampling, truncate=False,
                           batch_size=B)
    gt0 = s.gt_images[0]
    assert gt0[0, 4] == np.float32(4.7) and gt0[-1, 9] == np.float32(9.3)
    if sampling == "pool":
        ref_rule = DevicePatchSampler(train, device=None, sampling="pool", batch_size=B)
        on_edge = sum(int(((np.trunc(g) <= np.arange(W)) & (g > np.arange(W)) & np.isfinite(g)).sum()) for g in s.gt_images)
        assert on_edge == 2 * 40 and ref_rule.n_valid == s.n_valid + on_edge
        assert not (s.valid_gt > s.valid_col).any()
        batches = s.steps_per_epoch                      # the whole epoch: every valid pixel once
    else:
        batches = 2
    for _ in range(batches):
        rec = _returns(lambda: s.draw(B))
        left, pos, neg = rec[:B], rec[B:2 * B], rec[2 * B:]
        g = np.array([s.gt_images[int(i) // 2][int(r), int(c)] for i, r, c in zip(left["image"], left["cy"], left["cx"])])
        assert (g <= left["cx"]).all() and (g != np.round(g)).all()
        true = left["cx"].astype(np.float64) - g
        assert (np.abs(pos["cx"] - true) <= 0.5 + 1e-4).all()
        assert ((np.abs(neg["cx"] - true) >= 1.5 - 1e-4) & (np.abs(neg["cx"] - true) <= 6 + 1e-4)).all()
        for part in (pos, neg):
            assert ((part["cx"] >= 0) & (part["cx"] <= W - 1)).all()
    # the shared helper itself, on a row whose only candidates are such pixels and their neighbours
    gt = np.full((8, 12), np.inf, np.float32)
    gt[:, 4], gt[:, 5] = 4.7, 4.7                        # column 4: col - gt = -0.7; column 5: +0.3
    rows, cols, pos_col, neg_col = _returns(lambda: draw_pair_centres(np.random.default_rng(0), gt, 8, 0.5, 1.5, 6,
                                                                      truncate=False))
    assert (cols == 5).all() and (np.abs(pos_col - 0.3) <= 0.5 + 1e-6).all() and (pos_col >= 0).all()
    # ... which the truncating rule keeps, and ends on: int(4 - 4 + U(-0.5, 0.5)) = 0
    rows, cols, pos_col, neg_col = _returns(lambda: draw_pair_centres(np.random.default_rng(0), gt, 8, 0.5, 1.5, 6))
    assert set(cols) == {4, 5} and set(pos_col) <= {0, 1}


@pytest.mark.parametrize("preset", ["AUGMENT_MIDDLEBURY", "AUGMENT_KITTI"])
def test_augmentation_draws(tmp_path, preset):
    import datagenerator as dg
    a = getattr(dg, preset)
    assert sorted(a) == sorted(dg.AUGMENT_KEYS)
    lists = _write_dataset(str(tmp_path), seed=8)
    s = dg.DevicePatchSampler(os.path.join(lists, "train.txt"), rng=np.random.default_rng(4), device=None,
                              sampling="pool", augment=a, batch_size=200)
    B = 200
    rec = s.draw(B)
    q = s.last_params
    left, pos, neg = rec[:B], rec[B:2 * B], rec[2 * B:]
    eps = 1e-12
    # every drawn quantity in its stated interval
    assert (q["s"] >= a["scale"] - eps).all() and (q["s"] <= 1 + eps).all() and np.array_equal(q["sy"], q["s"])
    assert (q["sx"] >= a["scale"] * a["hscale"] - eps).all() and (q["sx"] <= q["s"] + eps).all()
    assert (np.abs(q["sh"]) <= a["hshear"] + eps).all()
    assert (np.abs(q["tx"]) <= a["trans"] + eps).all() and (np.abs(q["ty"]) <= a["trans"] + eps).all()
    assert (np.abs(q["phi"]) <= a["rotate"] * np.pi / 180 + eps).all()
    assert (np.abs(q["b"]) <= a["brightness"] + eps).all()
    assert (q["k"] >= 1. / a["contrast"] - eps).all() and (q["k"] <= a["contrast"] + eps).all()
    # left and right of a triplet differ by no more than the d_* bounds
    ratio = q["sx_r"] / q["sx"]
    assert (ratio >= a["d_hscale"] - 1e-9).all() and (ratio <= 1 + 1e-9).all()
    assert (np.abs(q["sh_r"] - q["sh"]) <= a["d_hshear"] + eps).all()
    assert (np.abs(q["ty_r"] - q["ty"]) <= a["d_vtrans"] + eps).all()
    assert (np.abs(q["phi_r"] - q["phi"]) <= a["d_rotate"] * np.pi / 180 + eps).all()
    assert (np.abs(q["b_r"] - q["b"]) <= a["d_brightness"] + eps).all()
    kr = q["k_r"] / q["k"]
    assert (kr >= 1. / a["d_contrast"] - 1e-9).all() and (kr <= a["d_contrast"] + 1e-9).all()
    # the records carry them: A . m = identity, gain k, bias b, the right patches share one draw
    for part, sx, sh, phi, k, b, ty in ((left, q["sx"], q["sh"], q["phi"], q["k"], q["b"], q["ty"]),
                                        (pos, q["sx_r"], q["sh_r"], q["phi_r"], q["k_r"], q["b_r"], q["ty_r"]),
                                        (neg, q["sx_r"], q["sh_r"], q["phi_r"], q["k_r"], q["b_r"], q["ty_r"])):
        A = dg.augment_matrix(sx, q["sy"], sh, phi)
        prod = A @ part["m"].astype(np.float64).reshape(B, 2, 2)
        assert np.abs(prod - np.eye(2)).max() <= 1e-6
        assert np.array_equal(part["gain"], k.astype(np.float32)) and np.array_equal(part["bias"], b.astype(np.float32))
        assert np.abs(np.round(part["cy"] + ty.astype(np.float32)) - (part["cy"] + ty.astype(np.float32))).max() <= 1e-4
    assert np.array_equal(pos["m"], neg["m"]) and np.array_equal(pos["cy"], neg["cy"])
    # the forward map is Shear . Rot . diag, x first: a point on the source x axis lands at (cos - sh sin, -sin) * sx
    A = dg.augment_matrix(0.5, 1.0, 0.25, np.pi / 6)
    c, sn = np.cos(np.pi / 6), np.sin(np.pi / 6)
    assert np.allclose(A, [[(c - 0.25 * sn) * 0.5, sn + 0.25 * c], [-sn * 0.5, c]])


def test_degenerate_augmentation_gives_identity_records(tmp_path):
    import datagenerator as dg
    lists = _write_dataset(str(tmp_path), seed=9)
    train = os.path.join(lists, "train.txt")
    plain = dg.DevicePatchSampler(train, rng=np.random.default_rng(5), device=None, sampling="pool", batch_size=64)
    aug = dg.DevicePatchSampler(train, rng=np.random.default_rng(5), device=None, sampling="pool", batch_size=64,
                                augment=dict(dg.AUGMENT_NONE))
    a, b = plain.draw(64), aug.draw(64)                   # the augmentation draws come after the centres
    assert a.tobytes() == b.tobytes()
    assert (b["m"] == (1, 0, 0, 1)).all() and not np.signbit(b["m"]).any()
    assert (b["gain"] == 1).all() and (b["bias"] == 0).all() and (b["cy"] == np.round(b["cy"])).all()
    with pytest.raises(ValueError):
        dg.DevicePatchSampler(train, device=None, augment={"rotation": 3})


def test_draw_refuses_an_image_outside_the_pool(tmp_path):
    from datagenerator import DevicePatchSampler
    lists = _write_dataset(str(tmp_path), seed=10)
    s = DevicePatchSampler(os.path.join(lists, "train.txt"), rng=np.random.default_rng(6), device=None, sampling="pool",
                           batch_size=16)
    rec = s.draw(16)
    with pytest.raises(Exception, match="no CPU fallback"):
        s.cut(rec)                                        # device=None draws and never cuts
    s.image_table = s.image_table[:2]                     # a pool of pair 0 alone under a table that names pair 1 too
    s.valid_pair[:] = 1
    with pytest.raises(ValueError, match="outside the pool"):
        s.draw(16)


def test_sample_patches_refusals_without_gpu():
    import _hipabi
    lib = _hipabi.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: the entry point validates before it launches
    assert lib.mccnn_sample_patches(None, None, 1, None, 1, 11, None, None) == _hipabi.MCCNN_E_INVALID == -1
    assert b"null pointer" in lib.mccnn_last_error_string()
    assert lib.mccnn_sample_patches(p, p, 1, p, 1, 11, None, None) == -1
    assert b"null pointer" in lib.mccnn_last_error_string()
    assert lib.mccnn_sample_patches(p, p, 1, p, 1, 10, p, None) == -1
    assert b"ps=10" in lib.mccnn_last_error_string()
    assert lib.mccnn_sample_patches(p, p, 1, p, 1, -3, p, None) == -1
    assert lib.mccnn_sample_patches(p, p, 1, p, 0, 11, p, None) == -1
    assert lib.mccnn_sample_patches(p, p, 0, p, 1, 11, p, None) == -1
    assert lib.mccnn_sample_patches(p, p, 1, p, 1, 33, p, None) == _hipabi.MCCNN_E_UNSUPPORTED == -2
    from datagenerator import SAMPLE_DTYPE, SAMPLE_IMAGE_DTYPE
    assert SAMPLE_DTYPE.itemsize == 36 and SAMPLE_IMAGE_DTYPE.itemsize == 16
    assert [SAMPLE_DTYPE.fields[n][1] for n in SAMPLE_DTYPE.names] == [0, 4, 8, 12, 28, 32]


@pytest.mark.parametrize("flags, named", [
    (["--sampling", "pool"], "--sampling pool"),
    (["--augment", "middlebury"], "--augment"),
    (["--subpixel_centres"], "--subpixel_centres"),
    (["--aug_rotate", "5"], "--aug_rotate"),
])
def test_parser_requires_the_device_sampler(flags, named, capsys):
    import train
    base = ["--list_dir", "l", "--tensorboard_dir", "t", "--checkpoint_dir", "c"]
    with pytest.raises(SystemExit) as e:
        train.parse_args(base + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert named in err and "--sampler device" in err
    args = train.parse_args(base + flags + ["--sampler", "device"])
    assert args.sampler == "device"
    plain = train.parse_args(base)
    assert plain.sampler == "host" and plain.sampling == "pair" and plain.augment == "none"
    assert plain.lr_drop_epoch is None and not plain.subpixel_centres and plain.augment_overrides == {}


@pytest.mark.parametrize("arch", ["fast", "accurate"])
def test_step_stacked_is_step(arch):
    import train
    from model import ACCURATE_NET, NET
    rng = np.random.default_rng(0)
    batch = [rng.standard_normal((6, 11, 11, 1)).astype(np.float32) for _ in range(3)]
    make = (lambda: ACCURATE_NET(None, batch_size=6, device="cpu", seed=1)) if arch == "accurate" else \
        (lambda: NET(None, batch_size=6, device="cpu", seed=1))
    a, b = train.Trainer(make(), 0.05, 0.9, 0.2), train.Trainer(make(), 0.05, 0.9, 0.2)
    x = torch.cat([torch.from_numpy(t) for t in batch])
    for _ in range(2):
        la, lb = a.step(*batch), b.step_stacked(x, 6)
        assert la == lb
    assert torch.equal(a.loss(*batch), b.loss_stacked(x, 6))
    for p, q in zip(a.params, b.params):
        assert torch.equal(p.detach(), q.detach())
