"""CPU: the accurate MC-CNN network (model.ACCURATE_NET) - patch forward, checkpoints, the BCE training step, the
library route of the decision stage, the command lines and the ABI additions - against the float64 restatements of
tests/accurate_reference.py."""
import os

import numpy as np
import pytest
import torch

import accurate_reference as ar
from conftest import GOLDEN_DIR

import tolerances


def _net(seed=3, **kw):
    from model import ACCURATE_NET
    kw.setdefault("device", "cpu")
    return ACCURATE_NET(None, seed=seed, **kw)


def test_patch_forward_matches_float64():
    """ReLU after every conv layer, no normalisation, n_fc ReLU layers, a units -> 1 layer, a sigmoid."""
    rng = np.random.default_rng(0)
    for kw in (dict(), dict(input_patch_size=9, num_conv_layers=4, num_fc_layers=4, num_conv_feature_maps=64)):
        net = _net(**kw)
        p = net.input_patch_size
        left = rng.standard_normal((7, p, p, 1)).astype(np.float32)
        right = rng.standard_normal((7, p, p, 1)).astype(np.float32)
        conv, fc = ar.net_lists(net)
        assert len(fc) == net.num_fc_layers + 1 and tuple(fc[0][0].shape) == (384, 2 * net.num_conv_feature_maps)
        assert tuple(fc[-1][0].shape) == (1, 384)
        want = ar.patch_scores_float64(conv, fc, left, right).numpy()
        got = net.scores(left, right).detach().numpy()
        assert got.shape == (7,) and got.dtype == np.float32
        assert np.abs(got - want).max() <= tolerances.ACCURATE_SCORE_ABS
        assert 0.0 < got.min() and got.max() < 1.0
        # the tower's output is what ReLU leaves: no negative value, no unit norm
        f = net(left).detach().numpy()
        assert f.shape == (7, 1, 1, net.num_conv_feature_maps) and f.min() >= 0.0
        assert np.abs(np.linalg.norm(f.reshape(7, -1), axis=1) - 1.0).min() > 1e-3
        ft = ar.tower_float64(conv, torch.from_numpy(left).permute(0, 3, 1, 2)).reshape(7, -1).numpy()
        assert np.abs(f.reshape(7, -1) - ft).max() <= tolerances.ACCURATE_SCORE_ABS


def test_checkpoint_round_trip(tmp_path):
    import tf_checkpoint
    from model import NET
    net = _net(seed=5, num_fc_layers=4)
    path = str(tmp_path / "acc.npz")
    net.save(path)
    z = np.load(path)
    assert sorted(k for k in z.files if k.startswith("fc")) == sorted(
        "fc%d/%s" % (k, n) for k in range(1, 6) for n in ("weights", "biases"))
    assert z["fc1/weights"].shape == (224, 384) and z["fc5/weights"].shape == (384, 1) and z["fc5/biases"].shape == (1,)
    assert z["conv2/weights"].shape == (3, 3, 112, 112)
    back = _net(seed=6, num_fc_layers=4).restore(path)
    for a, b in zip(net.fc_weights + net.fc_biases + net.weights + net.biases,
                    back.fc_weights + back.fc_biases + back.weights + back.biases):
        assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        _net(num_fc_layers=3).restore(path)
    # a fast checkpoint loads as before, and is refused as an accurate one
    fast = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
    layers = tf_checkpoint.load_fast_net_weights(fast)
    assert len(layers) == 5 and layers[1][0].shape == (3, 3, 64, 64)
    NET(None, device="cpu").restore(fast)
    with pytest.raises(ValueError):
        tf_checkpoint.load_accurate_net_weights(fast)
    # save_npz without fc layers writes what it always wrote
    tf_checkpoint.save_npz(str(tmp_path / "fast.npz"), layers)
    assert sorted(np.load(str(tmp_path / "fast.npz")).files) == sorted(
        "conv%d/%s" % (k, n) for k in range(1, 6) for n in ("weights", "biases"))
    # the conv part of an accurate checkpoint reads through the fast loader too
    assert len(tf_checkpoint.load_fast_net_weights(path)) == 5


def test_bce_training_step_matches_float64():
    """One Trainer.step under BCE: loss = mean(-log s+) / mean(-log(1 - s-)) over both halves, update var -= lr * grad
    (first momentum step), against a float64 evaluation of loss and gradients."""
    import train
    rng = np.random.default_rng(1)
    B = 5
    batch = [rng.standard_normal((B, 11, 11, 1)).astype(np.float32) for _ in range(3)]
    net = _net(seed=2, batch_size=B)
    conv, fc = ar.net_lists(net)
    params = [t.clone().double().requires_grad_(True) for pair in conv + fc for t in pair]
    conv64 = [(params[2 * k], params[2 * k + 1]) for k in range(len(conv))]
    fc64 = [(params[2 * (len(conv) + k)], params[2 * (len(conv) + k) + 1]) for k in range(len(fc))]

    def tower(x):
        x = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        for w, b in conv64:
            x = torch.relu(torch.nn.functional.conv2d(x, w, b))
        return x.reshape(B, -1)

    def score(a, b):
        x = torch.cat((a, b), -1)
        for k, (w, bb) in enumerate(fc64):
            x = torch.nn.functional.linear(x, w, bb)
            if k < len(fc64) - 1:
                x = torch.relu(x)
        return torch.sigmoid(x[:, 0])

    fl, fp, fn = (tower(b) for b in batch)
    want = (-torch.log(score(fl, fp)).sum() - torch.log(1 - score(fl, fn)).sum()) / (2 * B)
    want.backward()
    lr = 0.05
    t = train.Trainer(net, lr, 0.9, 0.2)
    got = t.step(*batch)
    assert abs(got - float(want.detach())) <= 1e-5
    now = [p for k in range(len(conv)) for p in (net.weights[k], net.biases[k])] + \
          [p for k in range(len(fc)) for p in (net.fc_weights[k], net.fc_biases[k])]
    moved = 0.0
    for p64, p in zip(params, now):
        expect = p64.detach() - lr * p64.grad
        assert (p.detach().double() - expect).abs().max() <= 1e-5
        moved = max(moved, float((lr * p64.grad).abs().max()))
    assert moved > 1e-4                    # the step is not a no-op the tolerance would hide
    # the checkpoint state carries the fc variables and their momentum slots
    st = t.state()
    assert st["fc1/weights"].shape == (224, 384) and st["fc4/weights/Momentum"].shape == (384, 1)


def test_train_cli_accurate_writes_npz_and_bce_scalars(tmp_path):
    import json
    import train
    from test_train_cpu import _write_dataset
    lists = _write_dataset(str(tmp_path), n_pairs=3, seed=2)
    log, ck = str(tmp_path / "log"), str(tmp_path / "ck")
    train.main(["--list_dir", lists, "--tensorboard_dir", log, "--checkpoint_dir", ck, "-bs", "8", "--arch", "accurate",
                "--end_epoch", "2", "--print_freq", "1", "--save_freq", "2", "--val_freq", "2"])
    tags = {json.loads(x)["tag"] for x in open(os.path.join(log, "scalars.jsonl"))}
    assert tags == {"bce_loss", "val_bce_loss"}
    path = os.path.join(ck, "model_epoch2.ckpt.npz")
    net = _net().restore(path)
    assert net.fc_weights[0].shape == (384, 224)
    train.main(["--list_dir", lists, "--tensorboard_dir", log, "--checkpoint_dir", ck, "-bs", "8", "--arch", "accurate",
                "--resume", path, "--start_epoch", "2", "--end_epoch", "3"])
    assert os.path.isfile(os.path.join(ck, "model_epoch3.ckpt.npz"))


def test_library_route_scores_on_cpu_tensors():
    """stereo_device.accurate_scores_library (what cost_volume_accurate(decision="library") runs before the fill
    launch) is plain torch: on CPU tensors, every w >= d score against the float64 restatement, both layouts, with a
    byte budget small enough to force row bands."""
    import stereo_device as sd
    net = _net(seed=7)
    H, W, D, C = 5, 23, 9, 112
    g = torch.Generator().manual_seed(0)
    fl = torch.relu(torch.randn((H, W, C), generator=g))
    fr = torch.relu(torch.randn((H, W, C), generator=g))
    _conv, fc = ar.net_lists(net)
    s64, e32, _e16 = ar.yardsticks(fc, fl, fr, D)
    m = ar.valid_mask(D, H, W)
    aL, aR = net.first_layer_halves(fl, fr)
    for pixel_major in (False, True):
        shape = (H, W, sd.hwd_pitch(D)) if pixel_major else (D, H, W)
        lcv, rcv = torch.full(shape, 7.0), torch.full(shape, 7.0)
        sd.accurate_scores_library(net, aL, aR, D, lcv, rcv, pixel_major, budget=3 * W * 384 * 4)
        l = lcv[:, :, :D].permute(2, 0, 1).numpy() if pixel_major else lcv.numpy()
        r = rcv[:, :, :D].permute(2, 0, 1).numpy() if pixel_major else rcv.numpy()
        assert np.abs(-l - s64)[m].max() <= tolerances.ACCURATE_SPLIT_E32_FACTOR * e32
        assert (l[~m] == 7.0).all()                              # borders are the fill launch's
        for d in range(D):
            assert np.array_equal(r[d, :, :W - d], l[d, :, d:])   # rcv[d,h,w] = lcv[d,h,w+d]
            assert (r[d, :, W - d:] == 7.0).all()


def test_border_restatement_is_the_fast_networks(golden_cases):
    """The literal float32 recurrences of accurate_reference.volumes_from_scores, applied to the w >= d costs of the
    fast network's golden pairs (recorded from the reference), give the recorded volumes bit for bit: the accurate
    network shares its borders and its right-volume copy with the fast one."""
    import helpers
    for name, g in golden_cases:
        l, r = ar.volumes_from_scores(g["cv_l"])
        helpers.assert_bits_strict(l, g["cv_l"], "%s: left borders" % name)
        helpers.assert_bits_strict(r, g["cv_r"], "%s: right volume" % name)


def test_cli_flags():
    import match
    import train
    base = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]
    a = match.parser.parse_args(base)
    assert a.arch == "fast" and a.num_fc_layers == 3 and a.decision == "auto"
    a = match.parser.parse_args(base + ["--arch", "accurate", "--num_fc_layers", "4"])
    assert a.arch == "accurate" and a.num_fc_layers == 4
    with pytest.raises(SystemExit):
        match.parser.parse_args(base + ["--arch", "medium"])
    tb = ["--list_dir", "l", "--tensorboard_dir", "t", "--checkpoint_dir", "c"]
    assert train.parser.parse_args(tb).arch == "fast"
    a = train.parser.parse_args(tb + ["--arch", "accurate", "--num_fc_layers", "4"])
    assert a.arch == "accurate" and a.num_fc_layers == 4


def test_abi_additions_and_refusals_without_gpu():
    """The new symbols are in the built library, the ABI is still 7, and the entry points refuse shapes outside the
    envelope before they launch (this runs without a GPU), naming the limit."""
    import _hipabi
    lib = _hipabi.load()
    assert lib.mccnn_version() == 7 and _hipabi.MCCNN_ABI_VERSION == 7
    for name in ("mccnn_decision_pack", "mccnn_decision_pack_bytes", "mccnn_cost_volume_accurate",
                 "mccnn_cost_volume_accurate_hwd", "mccnn_cost_volume_fill"):
        assert name in _hipabi.SIGNATURES and hasattr(lib, name)
    assert lib.mccnn_decision_pack_bytes(3, 384, 0) == 2 * 384 * 384 * 4      # two layers, hi + lo f16 per weight
    assert lib.mccnn_decision_pack_bytes(4, 384, 1) == 3 * 384 * 384 * 2
    assert lib.mccnn_decision_pack_bytes(3, 256, 0) == 0 and lib.mccnn_decision_pack_bytes(5, 384, 0) == 0
    one = 1          # any non-null address: validation comes before every use
    for fn in (lib.mccnn_cost_volume_accurate, lib.mccnn_cost_volume_accurate_hwd):
        def call(H=8, W=40, C=112, units=384, n_fc=3, D=16):
            return fn(one, one, H, W, C, units, n_fc, D, one, one, one, 0.0, 1.0, one, one, 0, None, None)
        assert call(C=96) == _hipabi.MCCNN_E_UNSUPPORTED and b"64 or 112" in lib.mccnn_last_error_string()
        assert call(units=256) == _hipabi.MCCNN_E_UNSUPPORTED and b"384" in lib.mccnn_last_error_string()
        assert call(n_fc=5) == _hipabi.MCCNN_E_UNSUPPORTED and b"3 or 4" in lib.mccnn_last_error_string()
        assert call(D=39) == _hipabi.MCCNN_E_UNSUPPORTED and b"W >= D+2" in lib.mccnn_last_error_string()
        assert call(W=2000, D=1025) == _hipabi.MCCNN_E_UNSUPPORTED and b"1024" in lib.mccnn_last_error_string()
        assert fn(None, one, 8, 40, 112, 384, 3, 16, one, one, one, 0.0, 1.0, one, one, 0, None, None) == -1
    # the Python-side statement of the same envelope
    import stereo_device as sd
    assert sd.decision_kernel_refusal(_net(), 40, 16) is None
    assert "96 feature maps" in sd.decision_kernel_refusal(_net(num_conv_feature_maps=96), 40, 16)
    assert "256 units" in sd.decision_kernel_refusal(_net(num_fc_units=256), 40, 16)
    assert "ndisp + 2" in sd.decision_kernel_refusal(_net(), 40, 39)
    assert sd.workspace_bytes(20, 40, 16, arch="accurate") - sd.workspace_bytes(20, 40, 16) == 2 * 20 * 40 * 384 * 4
