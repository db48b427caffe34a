"""GPU: mccnn_sample_patches against its NumPy restatement as uint32 patterns, DevicePatchSampler against
ImageDataGenerator (pair mode, same seed, same bits) and against the restatement (pool mode, augmented), and train.py
with the device sampler end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import patch_sampler_reference as ref
from conftest import ROOT
from test_patch_sampler_cpu import _write_dataset

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (12, 9), (40, 72)]
TRAIN = os.path.join(ROOT, "mc-cnn-python_amd", "src", "train.py")
MATCH = os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py")


@pytest.fixture(scope="module")
def pool():
    """(host images, device pool, device image table) of the three test images, -0.0 planted in each."""
    import torch
    from datagenerator import SAMPLE_IMAGE_DTYPE
    images = ref.planted_images(SHAPES, seed=1)
    table = np.zeros(len(images), dtype=SAMPLE_IMAGE_DTYPE)
    offset = 0
    for k, im in enumerate(images):
        table[k] = (offset, im.shape[0], im.shape[1])
        offset += im.size
    flat = np.concatenate([im.ravel() for im in images])
    return images, torch.from_numpy(flat).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()


def _launch(pool, rec, ps):
    import torch
    import _hipabi as hip
    _images, flat, table = pool
    out = torch.full((len(rec), ps, ps), float("nan"), dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(rec.view(np.uint8)).cuda()
    hip.check(hip.load().mccnn_sample_patches(hip.ptr(flat), hip.ptr(table), len(SHAPES), hip.ptr(dev), len(rec), ps,
                                              hip.ptr(out), hip.stream()), "mccnn_sample_patches")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 385])
@pytest.mark.parametrize("ps", [1, 3, 9, 11, 13, 31])
def test_kernel_is_the_restatement(pool, ps, N):
    rec = ref.mixed_records(SHAPES, N, ps, seed=1000 * ps + N)
    got = _launch(pool, rec, ps)
    helpers.assert_bits_strict(got, ref.sample_patches_arrays(pool[0], rec, ps), "ps=%d N=%d, array restatement" % (ps, N))
    some = np.unique(np.linspace(0, N - 1, min(N, 14)).astype(int))      # one of every kind, per pixel
    helpers.assert_bits_strict(got[some], ref.sample_patches(pool[0], rec[some], ps), "ps=%d N=%d, per pixel" % (ps, N))


def test_kernel_covers_more_patches_than_a_grid_dimension(pool):
    N = 65537
    rec = ref.mixed_records(SHAPES, N, 1, seed=77)
    got = _launch(pool, rec, 1)
    helpers.assert_bits_strict(got, ref.sample_patches_arrays(pool[0], rec, 1), "ps=1 N=65537")
    assert not np.isnan(got[-1]).any() and np.count_nonzero(got) > N // 4


def test_pair_mode_is_image_data_generator(tmp_path):
    from datagenerator import DevicePatchSampler, ImageDataGenerator
    lists = _write_dataset(str(tmp_path), seed=5)
    train = os.path.join(lists, "train.txt")
    g = ImageDataGenerator(train, shuffle=True, rng=np.random.default_rng(11))
    s = DevicePatchSampler(train, shuffle=True, rng=np.random.default_rng(11), device="cuda", sampling="pair")
    assert s.steps_per_epoch == 2
    for step in range(2):
        want = np.concatenate(g.next_batch(32))
        got = s.next_batch(32)
        assert got.is_cuda and tuple(got.shape) == (96, 11, 11, 1)
        helpers.assert_bits_strict(got.cpu().numpy(), want, "pair mode, batch %d" % step)


def test_pool_mode_augmented_is_the_restatement(tmp_path):
    import datagenerator as dg
    lists = _write_dataset(str(tmp_path), seed=6)
    s = dg.DevicePatchSampler(os.path.join(lists, "train.txt"), rng=np.random.default_rng(12), device="cuda",
                              sampling="pool", augment=dg.AUGMENT_MIDDLEBURY, truncate=False, batch_size=32)
    images = [im for pair in zip(s.left_images, s.right_images) for im in pair]
    for step in range(2):
        got = s.next_batch(32).cpu().numpy()
        rec = s.last_records
        assert got.shape == (96, 11, 11, 1) and len(rec) == 96 and (rec["m"][:, 1] != 0).any()
        helpers.assert_bits_strict(got[..., 0], ref.sample_patches_arrays(images, rec, 11), "pool mode, batch %d" % step)
        helpers.assert_bits_strict(got[::8, :, :, 0], ref.sample_patches(images, rec[::8], 11), "pool mode, per pixel")


def _train(tmp_path, lists, arch, extra):
    log, ck = str(tmp_path / ("log_" + arch)), str(tmp_path / ("ck_" + arch))
    cmd = [sys.executable, TRAIN, "-g", "0", "--list_dir", lists, "--tensorboard_dir", log, "--checkpoint_dir", ck,
           "--arch", arch, "--sampler", "device", "--sampling", "pool", "-bs", "32", "-lr", "0.05", "--end_epoch", "1",
           "--print_freq", "1", "--seed", "4"] + extra
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    tag = "bce_loss" if arch == "accurate" else "hinge_loss"
    pts = [json.loads(x) for x in open(os.path.join(log, "scalars.jsonl"))]
    losses = [p["value"] for p in pts if p["tag"] == tag]
    steps = [p["step"] for p in pts if p["tag"] == tag]
    val = [p for p in pts if p["tag"] == "val_" + tag]
    return losses, steps, val, os.path.join(ck, "model_epoch1.ckpt.npz")


def _n_valid(lists):
    from datagenerator import DevicePatchSampler
    return DevicePatchSampler(os.path.join(lists, "train.txt"), device=None, sampling="pool").n_valid


@pytest.mark.parametrize("arch", ["fast", "accurate"])
def test_train_cli_pool_sampling_learns(tmp_path, arch):
    """The criterion of test_train_cli_learns_and_checkpoint_round_trips on the same data and learning rate, here over
    one pooled epoch (245 steps): the mean of the last tenth of the logged losses below 0.7 x the mean of the first
    tenth.  Measured on the CPU with the NumPy restatement as the cut, same list, batch size, learning rate and seed:
    fast 0.050 -> 0.012 (ratio 0.23); accurate 0.694 -> 0.454 (ratio 0.65) - the binary cross-entropy stays at ln 2
    for about 190 steps and falls in the last fifty, with the host sampler's pair batches just the same (0.694 -> 0.433
    over as many steps), so the accurate case passes with little room."""
    lists = _write_dataset(str(tmp_path), n_pairs=4, seed=2)
    losses, steps, val, _ckpt = _train(tmp_path, lists, arch, [])
    n_steps = _n_valid(lists) // 32
    assert n_steps > 100 and len(losses) == n_steps and steps == list(range(n_steps))
    assert [p["step"] for p in val] == [n_steps] and np.isfinite(val[0]["value"])
    tenth = n_steps // 10
    first, last = np.mean(losses[:tenth]), np.mean(losses[-tenth:])
    print("%s: %d steps, first tenth %.4f, last tenth %.4f, ratio %.3f" % (arch, n_steps, first, last, last / first))
    assert last < 0.7 * first, (first, last)


@pytest.mark.parametrize("arch", ["fast", "accurate"])
def test_train_cli_augmented_subpixel_runs_and_checkpoint_is_read(tmp_path, arch):
    """No learning criterion here: nobody has measured how fast noise textures are learnt under 28 degree rotations."""
    from model import ACCURATE_NET, NET
    import tf_checkpoint
    lists = _write_dataset(str(tmp_path), n_pairs=4, seed=2)
    losses, _steps, val, ckpt = _train(tmp_path, lists, arch, ["--augment", "middlebury", "--subpixel_centres"])
    assert len(losses) == _n_valid(lists) // 32 and np.isfinite(losses).all() and np.isfinite(val[0]["value"])
    net = (ACCURATE_NET if arch == "accurate" else NET)(None, device="cpu").restore(ckpt)
    conv = tf_checkpoint.load_accurate_net_weights(ckpt)[0] if arch == "accurate" else tf_checkpoint.load_fast_net_weights(ckpt)
    assert np.array_equal(net.get_layers()[2][0], conv[2][0])
    pair = tmp_path / "pair3"
    (pair / "calib.txt").write_text("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                                    "width=72\nheight=40\nndisp=16\nisint=0\nvmin=0\nvmax=16\ndyavg=0\ndymax=0\n")
    lst = tmp_path / "match_list.txt"
    lst.write_text("%s/im0.png\n" % pair)
    out = tmp_path / "out"
    cmd = [sys.executable, MATCH, "-g", "0", "--list_file", str(lst), "--data_dir", str(tmp_path), "--save_dir", str(out),
           "-t", "aug", "-s", "0", "-e", "1", "--arch", arch, "--resume", ckpt]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    assert (out / "submit_aug" / "pair3" / "disp0MCCNN.pfm").is_file()
