import contextlib

import numpy as np

_QNAN = np.uint32(0x7fc00000)


def _canonical_bits(a):
    """uint32 patterns of a float32 array with every NaN mapped to one pattern (sign and payload dropped): NumPy on the
    host and the GPU both return A quiet NaN for an invalid operation, but which payload / sign is not part of IEEE 754
    and differs between x86 (default NaN = negative quiet NaN) and gfx950 (positive)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = _QNAN
    return u


def bits_strict(a, b):
    """Bit-for-bit equality of two arrays.  float32: compared through their uint32 patterns, so +0.0 != -0.0; only NaN
    payloads are canonicalised (_canonical_bits)."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.array_equal(_canonical_bits(a), _canonical_bits(b)))
    return bool(np.array_equal(a, b))


def bits_equal(a, b):
    """The strict comparison (kept under the name the tests have always used; until round 6 it also let +0 == -0 pass)."""
    return bits_strict(a, b)


def bits_equal_up_to_zero_sign(a, b):
    """bits_strict() that lets +0.0 == -0.0 pass: only for the places listed in DESIGN.md section 2 where a sign of zero
    is known to differ from the reference and no consumer can see it."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        same = _canonical_bits(a) == _canonical_bits(b)
        same |= (a == b)
        return bool(same.all())
    return bool(np.array_equal(a, b))


def hp_of(g):
    return dict(zip([str(k) for k in g["hp_names"]], [float(v) for v in g["hp_values"]]))


def _describe(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s against %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
    if a.dtype == np.float32:
        ua, ub = _canonical_bits(a), _canonical_bits(b)
        differ = ua != ub
        zero_sign = differ & (a == b)
        with np.errstate(invalid="ignore"):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        mx = float(np.nanmax(d)) if np.isfinite(d).any() else float("nan")
        return "max abs diff %g, %d of %d patterns differ (%d of them only in the sign of a zero)" % (
            mx, int(differ.sum()), a.size, int(zero_sign.sum()))
    return "%d of %d differ" % (int((a != b).sum()), a.size)


def assert_bits_strict(a, b, what):
    assert bits_strict(a, b), "%s: not bit-identical (%s)" % (what, _describe(a, b))


def assert_bits(a, b, what):
    """Strict since round 6: uint32 patterns, signs of zeros included, NaN payloads canonicalised only."""
    assert_bits_strict(a, b, what)


class Tally(object):
    """Collects the comparisons of one stage or fixture so that every case runs and the failures are reported together:
    bits() for float32 (bits_strict), equal() for integer arrays (values and dtype), settle() asserts."""

    def __init__(self, what):
        self.what, self.failures, self.total = what, [], 0

    def bits(self, got, want, what):
        self.total += 1
        if not bits_strict(got, want):
            self.failures.append("%s: %s" % (what, _describe(got, want)))

    def equal(self, got, want, what):
        self.total += 1
        got, want = np.asarray(got), np.asarray(want)
        if got.dtype != want.dtype or not np.array_equal(got, want):
            self.failures.append("%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape))

    def check(self, ok, what):
        self.total += 1
        if not ok:
            self.failures.append(what)

    def settle(self, floor=1):
        assert not self.failures, "%s: %d of %d comparisons differ:\n%s" % (self.what, len(self.failures), self.total,
                                                                            "\n".join(self.failures[:40]))
        assert self.total >= floor, "%s: %d comparisons, the matrix has %d" % (self.what, self.total, floor)


@contextlib.contextmanager
def module_setting(module, name, value):
    """Sets a module-level switch (process_functional.CBCA_ORDER, ...) for a block and puts back whatever stood there,
    so that no test decides which kernel a later test's un-set call reaches."""
    previous = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, previous)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def stagewise(keep, L, R, D, o, hp=None, features=None):
    """Feeds every stage output a matcher handed out through `keep` to the CPU checker's next stage (`o`: the oracle
    module; `hp`: the matcher's hyper-parameters, default match.py's).  Returns {stage: max |gpu - cpu|} in stage order
    (0.0 = all bits equal; a zero of the other sign counts as the smallest subnormal).  features=(fl, fr): the cost
    volume is checked against the oracle's from these features too."""
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    tau, dist = a["cbca_intensity"], a["cbca_distance"]
    d = {}

    def diff(x, y):
        x = _host(x)
        if bits_strict(x, y):
            return 0.0
        m = float(np.nanmax(np.abs(x.astype(np.float64) - y))) if x.shape == np.shape(y) else float("inf")
        return m if m > 0.0 else float(np.spacing(np.float32(0)))     # a zero of the other sign: not 'all bits equal'

    cv = [_host(t) for t in keep["cv"]]
    if features is not None:
        ocv = o.compute_cost_volume(_host(features[0]), _host(features[1]), D)
        d["cost_volume"] = max(diff(cv[0], ocv[0]), diff(cv[1], ocv[1]))
    c1 = o.cost_volume_aggregation(L, R, cv[0], cv[1], tau, dist, a["cbca_num_iterations1"])
    d["cbca_x%d" % a["cbca_num_iterations1"]] = max(diff(keep["cbca1"][0], c1[0]), diff(keep["cbca1"][1], c1[1]))
    g1 = [_host(t) for t in keep["cbca1"]]
    s = o.SGM_average(g1[0].copy(), g1[1].copy(), L, R, a["sgm_P1"], a["sgm_P2"], a["sgm_Q1"], a["sgm_Q2"], a["sgm_D"],
                      a["sgm_V"])
    d["sgm"] = max(diff(keep["sgm"][0], s[0]), diff(keep["sgm"][1], s[1]))
    gs = [_host(t) for t in keep["sgm"]]
    n2 = a["cbca_num_iterations2"]
    c2 = o.cost_volume_aggregation(L, R, gs[0], gs[1], tau, dist, n2)
    d["cbca_x%d" % n2] = max(diff(keep["cbca2"][0], c2[0]), diff(keep["cbca2"][1], c2[1]))
    d["cbca_x%d_spacings_of_max_input" % n2] = d["cbca_x%d" % n2] / float(np.spacing(np.float32(np.abs(gs[0]).max())))
    g2 = [_host(t) for t in keep["cbca2"]]
    dl, dr = o.disparity_prediction(g2[0], g2[1])
    gdl, gdr = _host(keep["wta"][0]), _host(keep["wta"][1])
    d["wta_mismatches"] = int((gdl != dl).sum() + (gdr != dr).sum())
    di = o.interpolation(gdl, gdr, D)
    d["interpolation"] = diff(keep["interp"], di)
    ds = o.subpixel_enhance(_host(keep["interp"]), g2[0])
    d["subpixel"] = diff(keep["subpixel"], ds)
    dm = o.median_filter(_host(keep["subpixel"]), 5, 5)
    d["median"] = diff(keep["median"], dm)
    db = o.bilateral_filter(L, _host(keep["median"]), 5, 5, 0, a["blur_sigma"], a["blur_threshold"])
    d["bilateral"] = diff(keep["bilateral"], db)
    return d


def first_differing_stage(d):
    """The first stage of a stagewise() record whose output differs from the CPU checker's, or None."""
    return next((k for k, v in d.items() if v != 0 and not k.endswith("_spacings_of_max_input")), None)


def features_float64(net, img, window=None):
    """[H,W] float32 image -> [H,W,64] float64 unit features by torch on the CPU: conv2d VALID on the once-padded image,
    ReLU, tf.nn.l2_normalize (model.py:51-64 of the reference as model.NET restates it).  window=(y0, y1, x0, x1):
    only the output pixels [y0:y1, x0:x1] - the padded image is cropped to the window's receptive field, so every
    pixel sees what it sees in the whole evaluation (it differs from it by at most 1.1e-16)."""
    import torch
    import torch.nn.functional as F
    pad = (net.input_patch_size - 1) // 2
    x = F.pad(img.double().cpu()[None, None], (pad, pad, pad, pad))
    if window is not None:
        y0, y1, x0, x1 = window
        x = x[:, :, y0:y1 + 2 * pad, x0:x1 + 2 * pad]
    nl = net.num_conv_layers
    for k in range(nl):
        x = F.conv2d(x, net.weights[k].detach().double().cpu(), net.biases[k].detach().double().cpu())
        if k < nl - 1:
            x = F.relu(x)
    x = x[0].permute(1, 2, 0)
    return x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))


def smooth_pair(H, W, seed):
    """Two standardised float32 [H,W] views: low-pass noise and its shifted, noisier copy."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    a = F.avg_pool2d(torch.randn((1, 1, H + 8, W + 8), generator=g), 5, 1, 2)[0, 0, 4:-4, 4:-4]
    b = torch.roll(a, 3, 1) + 0.05 * torch.randn((H, W), generator=g)
    out = []
    for t in (a, b):
        out.append(((t - t.mean()) / t.std()).float().contiguous())
    return out


def split_f16(v):
    """Already scaled float32 values inside the f16 range -> (hi, lo) float16 with hi = f16(v), lo = f16(v - hi)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def records_encode(x, act_scale):
    """float32 [..., 64] -> the 256-byte split records of include/mccnn.h, uint8 [..., 256]:
    [q = channel / 16][hi 16 x f16 | lo 16 x f16] of x * act_scale."""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] == 64
    hi, lo = split_f16(x * np.float32(act_scale))
    rec = np.empty(x.shape[:-1] + (4, 2, 16), np.float16)
    rec[..., 0, :] = hi.reshape(x.shape[:-1] + (4, 16))
    rec[..., 1, :] = lo.reshape(x.shape[:-1] + (4, 16))
    return rec.reshape(x.shape[:-1] + (128,)).view(np.uint8)


def records_decode(rec, act_scale):
    """Split records uint8 [..., 256] -> float32 [..., 64]: (hi + lo) / act_scale.  The sum is exact in float32 for
    records made from float32 values, and act_scale is a power of two."""
    rec = np.ascontiguousarray(rec)
    assert rec.dtype == np.uint8 and rec.shape[-1] == 256
    h = rec.view(np.float16).reshape(rec.shape[:-1] + (4, 2, 16))
    v = h[..., 0, :].astype(np.float32) + h[..., 1, :].astype(np.float32)
    return (v / np.float32(act_scale)).reshape(rec.shape[:-1] + (64,))
