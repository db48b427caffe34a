"""Restatements the accurate-network tests compare against, written from the paper's description (Zbontar & LeCun 2016,
sec. 3.2) - nothing here calls the code under test.

  * float64 (torch on the CPU): the tower (3x3 VALID convolutions on the once-padded image, ReLU after EVERY layer, no
    normalisation), the decision network on [fL(h,w) ; fR(h,w-d)] (n_fc layers of ReLU units, a units -> 1 layer, a
    sigmoid) and the scores s(h,w,d) for every w >= d;
  * the same decision network in float32 (E32) and in float64 with weights and every layer's input activations rounded
    to f16 (E16): the two error yardsticks of src/tolerances.py;
  * the decision network from the two halves of its first layer (what the kernel is handed, NaN and inf included),
    and scores and yardsticks on a sample of voxels that holds every seam of the kernel's tiling, for volumes too
    large to restate whole;
  * float32, literal: the two border recurrences and the right-volume copy of compute_cost_volume, which the accurate
    network shares with the fast one.
Networks are passed as plain lists: conv = [(w [Cout,Cin,3,3], b)], fc = [(w [out,in], b)] (torch layout, any dtype)."""
import numpy as np
import torch
import torch.nn.functional as F


def net_lists(net):
    """(conv, fc) lists of CPU tensors from a model.ACCURATE_NET."""
    conv = [(w.detach().cpu(), b.detach().cpu()) for w, b in zip(net.weights, net.biases)]
    fc = [(w.detach().cpu(), b.detach().cpu()) for w, b in zip(net.fc_weights, net.fc_biases)]
    return conv, fc


def tower_float64(conv, x_nchw):
    """x [B,1,h,w] (already padded where padding is wanted) -> [B,C,h-2n,w-2n] float64."""
    x = torch.as_tensor(x_nchw).double()
    for w, b in conv:
        x = F.relu(F.conv2d(x, w.double(), b.double()))
    return x


def image_features_float64(conv, img_hw):
    """[H,W] image -> [H,W,C] float64: zero-padded ONCE by the receptive field's half width."""
    pad = len(conv)
    x = F.pad(torch.as_tensor(img_hw).double()[None, None], (pad, pad, pad, pad))
    return tower_float64(conv, x)[0].permute(1, 2, 0).contiguous()


def _round16(t):
    return t.to(torch.float16).to(t.dtype)


def decision(fc, x, dtype=torch.float64, round16=False):
    """x [..., 2C] -> scores [...] in `dtype`; round16: weights and every layer's input rounded to f16."""
    x = torch.as_tensor(x).to(dtype)
    for k, (w, b) in enumerate(fc):
        w = w.to(dtype)
        if round16:
            w, x = _round16(w), _round16(x)
        x = F.linear(x, w, b.to(dtype))
        if k < len(fc) - 1:
            x = F.relu(x)
    return torch.sigmoid(x[..., 0])


def patch_scores_float64(conv, fc, left, right):
    """left, right: NHWC patch batches [B,p,p,1] -> [B] float64 scores."""
    fl = tower_float64(conv, torch.as_tensor(left).permute(0, 3, 1, 2)).reshape(len(left), -1)
    fr = tower_float64(conv, torch.as_tensor(right).permute(0, 3, 1, 2)).reshape(len(right), -1)
    return decision(fc, torch.cat((fl, fr), -1))


def scores(fc, fl, fr, D, dtype=torch.float64, round16=False):
    """fl, fr [H,W,C] -> float64 ndarray [D,H,W]: s(h,w,d) for w >= d evaluated in `dtype`, NaN where w < d."""
    fl, fr = torch.as_tensor(fl), torch.as_tensor(fr)
    H, W, _ = fl.shape
    out = np.full((D, H, W), np.nan, np.float64)
    with torch.no_grad():
        for d in range(D):
            x = torch.cat((fl[:, d:, :], fr[:, :W - d, :]), -1)
            out[d, :, d:] = decision(fc, x, dtype, round16).double().numpy()
    return out


def valid_mask(D, H, W):
    """[D,H,W] bool: w >= d."""
    return (np.arange(W)[None, None, :] >= np.arange(D)[:, None, None]) & np.ones((1, H, 1), bool)


def yardsticks(fc, fl, fr, D):
    """(S64, E32, E16) on these inputs: the float64 scores, the max error of the float32 evaluation and of the f16
    emulation over every w >= d."""
    s64 = scores(fc, fl, fr, D)
    m = valid_mask(D, *s64.shape[1:])
    e32 = float(np.abs(scores(fc, fl, fr, D, torch.float32) - s64)[m].max())
    e16 = float(np.abs(scores(fc, fl, fr, D, torch.float64, True) - s64)[m].max())
    return s64, e32, e16


def decision_from_halves(fc, aL_rows, aR_rows, dtype=torch.float64, round16=False):
    """What the decision kernel computes from ITS inputs: aL_rows, aR_rows [N, units], the first layer's two halves at
    N (pixel, pixel - d) pairs (aL = W1[:, :C] fL + b1, aR = W1[:, C:] fR) -> scores [N] in `dtype`:
    relu(aL + aR), layers 2 .. n_fc, the final layer, the sigmoid.  fc as everywhere (fc[0] is not used: the halves
    carry it).  round16: the weights and every layer's input rounded to f16, from layer 2 on.  Unlike decision(), which
    starts from the tower outputs, this can be fed halves that hold NaN or inf: IEEE arithmetic (relu(NaN) = NaN,
    relu(-inf) = 0, inf * 0 = NaN), i.e. what the library route gives."""
    x = F.relu(torch.as_tensor(aL_rows).to(dtype) + torch.as_tensor(aR_rows).to(dtype))
    for k, (w, b) in enumerate(fc[1:], start=1):
        w = w.to(dtype)
        if round16:
            w, x = _round16(w), _round16(x)
        x = F.linear(x, w, b.to(dtype))
        if k < len(fc) - 1:
            x = F.relu(x)
    return torch.sigmoid(x[..., 0])


def _nearest_at_or_above(d, residue):
    """The smallest w >= d with w % 4 == residue."""
    return d + (residue - d) % 4


def seam_voxels(H, W, D):
    """The (h, w, d) triples sample_voxels() must contain, as a sorted list: the seams of the decision kernel's tiling
    (32 disparities per wave, 4 pixels per workgroup, the diagonal w = d, the ragged last workgroup).  For every h:
    every d with d % 32 in {0, 31} and d = D - 1, each with w in {d, d+1, d+3, d+4, W-2, W-1} and the nearest w >= d
    with w % 4 == 0 and with w % 4 == 3 (those that are valid: d <= w < W)."""
    ds = sorted(set(d for d in range(D) if d % 32 in (0, 31)) | {D - 1})
    out = set()
    for d in ds:
        ws = {d, d + 1, d + 3, d + 4, W - 2, W - 1, _nearest_at_or_above(d, 0), _nearest_at_or_above(d, 3)}
        for w in ws:
            if d <= w < W:
                out.update((h, w, d) for h in range(H))
    return sorted(out)


def sample_voxels(H, W, D, n_random, seed):
    """(h, w, d) int64 index arrays of valid voxels (w >= d): seam_voxels(H, W, D), then n_random voxels drawn uniformly
    from all valid ones (seeded; a draw may repeat a voxel)."""
    rng = np.random.default_rng(seed)
    seams = np.array(seam_voxels(H, W, D), np.int64).reshape(-1, 3)
    got = []
    need = int(n_random)
    while need > 0:                              # rejection: uniform on the box, the w >= d part kept
        n = 2 * need + 16
        h, w, d = rng.integers(0, H, n), rng.integers(0, W, n), rng.integers(0, D, n)
        ok = w >= d
        got.append(np.stack((h[ok], w[ok], d[ok]), 1)[:need])
        need -= len(got[-1])
    hwd = np.concatenate([seams] + got, 0).astype(np.int64)
    return hwd[:, 0].copy(), hwd[:, 1].copy(), hwd[:, 2].copy()


def sampled_scores(fc, fl, fr, sample, dtype=torch.float64, round16=False):
    """scores() at the voxels of `sample` = (h, w, d) only: float64 ndarray [N]."""
    fl, fr = torch.as_tensor(fl), torch.as_tensor(fr)
    h, w, d = (torch.as_tensor(np.asarray(a, np.int64)) for a in sample)
    assert bool((w >= d).all())
    with torch.no_grad():
        x = torch.cat((fl[h, w, :], fr[h, w - d, :]), -1)
        return decision(fc, x, dtype, round16).double().numpy()


def sampled_yardsticks(fc, fl, fr, sample):
    """(S64 [N], E32, E16) at the voxels of `sample` = (h, w, d), with the definitions of yardsticks(): the float64
    scores, the max error of the float32 evaluation and of the f16 emulation over the sample."""
    s64 = sampled_scores(fc, fl, fr, sample)
    e32 = float(np.abs(sampled_scores(fc, fl, fr, sample, torch.float32) - s64).max())
    e16 = float(np.abs(sampled_scores(fc, fl, fr, sample, torch.float64, True) - s64).max())
    return s64, e32, e16


# The shapes at which the decision stage is run up to its documented limit of 1024 disparities (test_accurate_edges_*):
# name -> (H, W, D, feature maps, fc layers, patch)
EDGE_CASES = {
    "2x1026x1024": (2, 1026, 1024, 112, 3, 11),    # 32 disparity blocks, Dp = D
    "2x520x513": (2, 520, 513, 64, 4, 9),          # the last block holds one disparity, Dp = 516, W % 4 = 0
    "3x1003x769": (3, 1003, 769, 112, 3, 11),      # Dp = 772, W % 4 = 3
}
EDGE_RANDOM_VOXELS = 6000
EDGE_SAMPLE_CAP = 30000


def edge_sample(name):
    H, W, D = EDGE_CASES[name][:3]
    return sample_voxels(H, W, D, EDGE_RANDOM_VOXELS, seed=H + W + D)


def _mean3(a, b, c):
    """np.mean of three float32 values summed in this order: the reduction starts from +0 and adds one by one."""
    s = np.float32(0) + a
    s = s + b
    s = s + c
    return (s / np.float32(3)).astype(np.float32)


def volumes_from_scores(neg_scores):
    """neg_scores float32 [D,H,W] holding -s for w >= d (other entries ignored) -> (lcv, rcv) float32 [D,H,W]:
         on the positive scores p = s:   p[d,h,w] = mean(p[d,h,w+1], p[d,h,w+2], p[d,h,w+3])      w = d-1 .. 0
         right volume                    q[d,h,w] = p[d,h,w+d]                                     w < W-d
                                         q[d,h,w] = mean(q[d,h,w-3], q[d,h,w-2], q[d,h,w-1])      w = W-d .. W-1
         lcv = -p, rcv = -q (the volumes are negated after the borders are filled)."""
    p = -np.asarray(neg_scores, np.float32)
    D, H, W = p.shape
    q = np.zeros_like(p)
    for d in range(D):
        for w in range(d - 1, -1, -1):
            p[d, :, w] = _mean3(p[d, :, w + 1], p[d, :, w + 2], p[d, :, w + 3])
        q[d, :, :W - d] = p[d, :, d:]
        for w in range(W - d, W):
            q[d, :, w] = _mean3(q[d, :, w - 3], q[d, :, w - 2], q[d, :, w - 1])
    return -p, -q


def volumes_from_scores_by_column(neg_scores):
    """volumes_from_scores() with its loops exchanged: one step per border column, every disparity that has that column
    at once (D + D steps instead of D * D).  Each element goes through the same _mean3 of the same three elements, so the
    result is the same bit for bit (tests/test_accurate_edges_cpu.py); for volumes of many hundred disparities."""
    p = -np.asarray(neg_scores, np.float32)
    D, H, W = p.shape
    for w in range(D - 2, -1, -1):                # left border: w < d, from the diagonal outwards
        p[w + 1:, :, w] = _mean3(p[w + 1:, :, w + 1], p[w + 1:, :, w + 2], p[w + 1:, :, w + 3])
    q = np.zeros_like(p)
    for d in range(D):
        q[d, :, :W - d] = p[d, :, d:]
    for w in range(W - D + 1, W):                 # right border: w >= W - d
        q[W - w:, :, w] = _mean3(q[W - w:, :, w - 3], q[W - w:, :, w - 2], q[W - w:, :, w - 1])
    return -p, -q
