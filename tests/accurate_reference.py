"""Restatements the accurate-network tests compare against, written from the paper's description (Zbontar & LeCun 2016,
sec. 3.2) - nothing here calls the code under test.

  * float64 (torch on the CPU): the tower (3x3 VALID convolutions on the once-padded image, ReLU after EVERY layer, no
    normalisation), the decision network on [fL(h,w) ; fR(h,w-d)] (n_fc layers of ReLU units, a units -> 1 layer, a
    sigmoid) and the scores s(h,w,d) for every w >= d;
  * the same decision network in float32 (E32) and in float64 with weights and every layer's input activations rounded
    to f16 (E16): the two error yardsticks of src/tolerances.py;
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
