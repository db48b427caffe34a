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
    network shares with the fast one;
  * weight families (what a trained network may look like: layers of different magnitude, outliers, heavy tails,
    zeros, tiny, huge and non-finite weights), each a stated transform of the seeded glorot network (whose initial
    VALUES are read from model.ACCURATE_NET, nothing else), and a NumPy restatement of the decision kernel's operand
    format (split_emulation), to tell what the format loses from what the kernel loses.
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


# ---- weight families: what a trained network may look like, built from the seeded glorot network by a stated transform --
OPERAND_LIMIT = 65504.0 / 256.0          # 255.875: an activation beyond it is clamped and raises the saturation flag
PREMISE_LIMIT = OPERAND_LIMIT / 2        # every family keeps its float64 pre-activations below this on the test inputs

GAP_FAMILIES = ("gap_2^4", "gap_2^8", "gap_2^12")
LATE_GAP_FAMILY = "gap34_2^12"           # n_fc = 4 only: the gap between fc3 and fc4
SPREAD_FAMILIES = ("outlier_1e3", "lognormal", "laplace", "sparse_95")
TINY_FAMILIES = ("tiny_1e-30", "tiny_1e-34", "tiny_1e-38")
NONFINITE_FAMILIES = ("nonfinite_+inf", "nonfinite_-inf", "nonfinite_nan")
REFUSAL_FAMILIES = ("huge_1e30",) + NONFINITE_FAMILIES        # refusal and flag tests only


def score_families(n_fc):
    """The families whose scores are compared with float64, for a network of n_fc hidden layers."""
    return ("glorot",) + GAP_FAMILIES + ((LATE_GAP_FAMILY,) if n_fc == 4 else ()) + SPREAD_FAMILIES + TINY_FAMILIES


def glorot_lists(C, n_fc, seed, patch=None):
    """(conv, fc) of the seeded glorot ACCURATE_NET the GPU tests build (the initial values come from a CPU generator,
    so they are the same on every device)."""
    from model import ACCURATE_NET
    patch = patch if patch is not None else (11 if C == 112 else 9)
    net = ACCURATE_NET(None, input_patch_size=patch, num_conv_layers=(patch - 1) // 2, num_conv_feature_maps=C,
                       num_fc_layers=n_fc, batch_size=1, device="cpu", seed=seed)
    return net_lists(net)


def hidden_preactivation_max(fc, fl, fr, D):
    """(max of aL + aR, max over the hidden layers 2 .. n_fc of the pre-activation) in float64 over every w >= d;
    the largest VALUE, as the kernel's range test is one-sided.  Non-finite weights give non-finite maxima."""
    fl, fr = torch.as_tensor(fl).double(), torch.as_tensor(fr).double()
    W = fl.shape[1]
    first, hidden = -np.inf, -np.inf
    with torch.no_grad():
        for d in range(D):
            x = F.linear(torch.cat((fl[:, d:, :], fr[:, :W - d, :]), -1), fc[0][0].double(), fc[0][1].double())
            first = max(first, float(x.max()))
            x = F.relu(x)
            for w, b in fc[1:-1]:
                x = F.linear(x, w.double(), b.double())
                hidden = max(hidden, float(x.max()))
                x = F.relu(x)
    return first, hidden


def _halve_into_range(fc, n_fc, inputs):
    """Halves every hidden layer 2 .. n_fc (weights and biases) until the float64 pre-activations are below
    PREMISE_LIMIT on `inputs` = (fl, fr, D); returns the number of halvings."""
    n = 0
    while hidden_preactivation_max(fc, *inputs)[1] >= PREMISE_LIMIT:
        for k in range(1, n_fc):
            fc[k] = (fc[k][0] * 0.5, fc[k][1] * 0.5)
        n += 1
        assert n < 64
    return n


def weight_family(name, C, n_fc, seed, inputs=None, patch=None):
    """(conv, fc) lists shaped like ACCURATE_NET(C maps, n_fc hidden layers): the seeded glorot network with its HIDDEN
    layers fc 2 .. n_fc (the ones the decision kernel packs; list indices 1 .. n_fc - 1) transformed as `name` says.
    The tower, fc1 and the final layer are glorot's.  Every scaling between layers is an exact power of two and biases
    are scaled with their layer, so for the gap families the float64 network function IS glorot's.
      glorot                     the control
      gap_2^4 | gap_2^8 | gap_2^12   (W_2, b_2) / g and W_3 * g: the small layer first
      gap34_2^12                 n_fc = 4: (W_3, b_3) / g and W_4 * g
      outlier_1e3                one weight in 10^4 of every hidden layer (seeded positions) x 1000, then all hidden
                                 layers halved until the float64 pre-activations on `inputs` are below PREMISE_LIMIT
      lognormal                  random signs, magnitudes exp(N(mu, 2.5)) - four decades - at glorot's RMS, then halved
                                 the same way (mu is chosen by the RMS and the halvings); glorot's biases, halved along
      laplace                    Laplace-distributed weights of glorot's variance; halved the same way if need be
      sparse_95                  95 % of the weights exact zeros, every other one of them -0.0; the rest x 4
      tiny_1e-30 | _1e-34 | _1e-38   hidden weights glorot * (m / max |glorot|), biases glorot's.  (The hidden weights then
                                 add less than 1e-27 to a pre-activation of order 0.1: the scores are the biases' and the
                                 final layer's, the same for every voxel to float64's last bit.)
      huge_1e30                  hidden weights glorot * (1e30 / max), biases glorot's
      nonfinite_+inf | _-inf | _nan  one hidden weight (seeded position) replaced
    inputs = (fl, fr, D), needed by the families that are halved into range."""
    conv, fc = glorot_lists(C, n_fc, seed, patch)
    fc = [(w.clone(), b.clone()) for w, b in fc]
    rng = np.random.default_rng(1000 + seed)
    hidden = range(1, n_fc)
    if name == "glorot":
        pass
    elif name in GAP_FAMILIES or name == LATE_GAP_FAMILY:
        g = float(2 ** int(name.split("^")[1]))
        k = 1 if name in GAP_FAMILIES else 2
        assert k + 1 <= n_fc - 1, "%s needs another hidden layer" % name
        fc[k] = (fc[k][0] / g, fc[k][1] / g)
        fc[k + 1] = (fc[k + 1][0] * g, fc[k + 1][1])
    elif name == "outlier_1e3":
        for k in hidden:
            w = fc[k][0].clone()
            pos = rng.choice(w.numel(), size=max(1, w.numel() // 10000), replace=False)
            w.view(-1)[torch.from_numpy(pos)] *= 1000.0
            fc[k] = (w, fc[k][1])
        _halve_into_range(fc, n_fc, inputs)
    elif name in ("lognormal", "laplace"):
        for k in hidden:
            w0 = fc[k][0]
            rms = float(w0.double().pow(2).mean().sqrt())
            if name == "lognormal":
                v = rng.choice((-1.0, 1.0), size=tuple(w0.shape)) * np.exp(rng.normal(0.0, 2.5, size=tuple(w0.shape)))
            else:
                v = rng.laplace(0.0, 1.0, size=tuple(w0.shape))
            v *= rms / np.sqrt(np.mean(v * v))
            fc[k] = (torch.from_numpy(v.astype(np.float32)), fc[k][1])
        _halve_into_range(fc, n_fc, inputs)
    elif name == "sparse_95":
        for k in hidden:
            w = fc[k][0].clone() * 4.0
            zero = np.flatnonzero(rng.random(w.numel()) < 0.95)
            flat = w.view(-1)
            flat[torch.from_numpy(zero[0::2])] = 0.0
            flat[torch.from_numpy(zero[1::2])] = -0.0
            fc[k] = (w, fc[k][1])
    elif name in TINY_FAMILIES or name == "huge_1e30":
        m = float(name.split("_")[1])
        for k in hidden:
            w = fc[k][0].double()
            fc[k] = ((w * (m / float(w.abs().max()))).float(), fc[k][1])
    elif name in NONFINITE_FAMILIES:
        value = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[name.split("_")[1]]
        k = 1 + int(rng.integers(0, n_fc - 1))
        w = fc[k][0].clone()
        w.view(-1)[int(rng.integers(0, w.numel()))] = value
        fc[k] = (w, fc[k][1])
    else:
        raise ValueError("unknown weight family %r" % name)
    return conv, fc


def layer_maxima(fc):
    """max |w| of the hidden layers fc 2 .. n_fc."""
    return [float(w.abs().max()) for w, _b in fc[1:-1]]


# ---- the operand format of the decision kernel, restated in NumPy ------------------------------------------------------
EMU_ACT_SCALE = 256.0


def packing_rule_single_max(fc):
    """The packing rule the kernel shipped with: ONE power of two from the largest |w| of ALL hidden layers,
    2^floor(log2(1024 / m)), the layers as the network has them."""
    m = max(layer_maxima(fc))
    return float(2.0 ** np.floor(np.log2(1024.0 / m)))


def _split16(x32, flush):
    """float32 values inside the f16 range -> (hi, lo) as float64 arrays holding f16 values: hi = f16(x), lo =
    f16(x - hi) (round to nearest even, subnormals kept).  flush: f16 subnormals (|v| < 2^-14) read as 0."""
    x32 = np.clip(np.asarray(x32, np.float32), np.float32(-65504.0), np.float32(65504.0))
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    if flush:
        hi[np.abs(hi) < 2.0 ** -14] = 0.0
        lo[np.abs(lo) < 2.0 ** -14] = 0.0
    return hi, lo


def split_emulation(fc, fl, fr, D, scale=None, flush=False, f16=False):
    """The decision kernel's arithmetic on the layers `fc` AS GIVEN (fc[0]: the first layer, float32 products; fc[1:-1]:
    the packed layers; fc[-1]: the final layer) -> (scores float64 [D,H,W] with NaN where w < d, saturation flag).
    scale: the power of two the weights are packed with (default: packing_rule_single_max).  Per hidden layer:
    w * scale and x * 256 each as hi + lo in f16 (subnormals kept; flush=True: read as 0, the question DESIGN.md 4.7
    answers by measurement), the three products lo*hi + hi*lo + hi*hi one after the other per k-step of 16, each k-step's
    sixteen products summed exactly and added to a float32 accumulator, then acc * (1 / (scale * 256)) + bias in float32,
    the range test, ReLU.  f16: one product hi*hi per multiply (the kernel's other precision).  The final layer, the
    sigmoid: float32 (summation order is not the kernel's tree).  It tells "lost by the format" from "lost by the
    kernel" when a GPU case fails; it is not the kernel, and no GPU bound is taken from it."""
    fl, fr = np.asarray(fl, np.float32), np.asarray(fr, np.float32)
    H, W, C = fl.shape
    scale = np.float32(packing_rule_single_max(fc) if scale is None else scale)
    inv = np.float32(1.0) / np.float32(scale * np.float32(EMU_ACT_SCALE))
    w1, b1 = (np.asarray(t, np.float32) for t in fc[0])
    aL = fl.reshape(-1, C) @ w1[:, :C].T + b1
    aR = fr.reshape(-1, C) @ w1[:, C:].T
    aL, aR = aL.reshape(H, W, -1), aR.reshape(H, W, -1)
    x = np.concatenate([(aL[:, d:, :] + aR[:, :W - d, :]).reshape(-1, aL.shape[-1]) for d in range(D)], 0)
    flag = bool((~(x * np.float32(EMU_ACT_SCALE) <= np.float32(65504.0))).any())
    x = np.maximum(x, np.float32(0.0))
    hidden = fc[1:-1]
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (w, b) in enumerate(hidden):
            w_hi, w_lo = _split16(np.asarray(w, np.float32) * scale, flush)
            x_hi, x_lo = _split16(x * np.float32(EMU_ACT_SCALE), flush)
            acc = np.zeros((x.shape[0], w_hi.shape[0]), np.float32)
            for s in range(0, w_hi.shape[1], 16):
                k16 = slice(s, s + 16)
                terms = ((w_hi, x_hi),) if f16 else ((w_lo, x_hi), (w_hi, x_lo), (w_hi, x_hi))
                for wp, xp in terms:
                    acc = (acc.astype(np.float64) + xp[:, k16] @ wp[:, k16].T).astype(np.float32)
            x = acc * inv + np.asarray(b, np.float32)
            limit = np.float32(OPERAND_LIMIT) if k + 1 < len(hidden) else np.float32(np.inf)
            flag |= bool((~(x <= limit)).any())
            x = np.maximum(x, np.float32(0.0))
        z = x @ np.asarray(fc[-1][0], np.float32).reshape(-1) + np.float32(np.asarray(fc[-1][1]).reshape(-1)[0])
        s = (np.float32(1.0) / (np.float32(1.0) + np.exp(-z))).astype(np.float64)
    out = np.full((D, H, W), np.nan, np.float64)
    at = 0
    for d in range(D):
        n = H * (W - d)
        out[d, :, d:] = s[at:at + n].reshape(H, W - d)
        at += n
    return out, int(flag)
