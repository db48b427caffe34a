"""A literal restatement of the semi-dense definitions of include/mccnn.h - of the definitions, not of the kernel: the
selection as three boolean expressions, the components as a plain flood fill over the links, float32 arithmetic through
NumPy scalars."""
import numpy as np

NAMES = ("msm", "mmn", "cur", "lrc")
BITS = dict(msm=1, mmn=2, cur=4, lrc=8)
INF = np.float32(np.inf)


def valid(d):
    """Finite and >= 0; -0.0 is valid, NaN, -1 and +-inf are not."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= np.float32(0))


def select(disp, status=None, planes=None, plane_names=(), thresholds=None, require_match=False):
    """mccnn_semi_dense_select: planes [K,H,W] in the order of plane_names (ascending bit order), thresholds {name: min}."""
    disp = np.asarray(disp, np.float32)
    plane_names = tuple(plane_names)
    assert plane_names == tuple(n for n in NAMES if n in plane_names)
    is_valid = valid(disp)
    matched = np.ones(disp.shape, bool) if not require_match else np.asarray(status) == 0
    confident = np.ones(disp.shape, bool)
    for name, t in (thresholds or {}).items():
        with np.errstate(invalid="ignore"):
            confident &= np.asarray(planes[plane_names.index(name)], np.float32) >= np.float32(t)
    return np.where(is_valid & matched & confident, disp, INF).astype(np.float32)


def linked(a, b, max_diff):
    """Both valid and |a - b| <= max_diff: one float32 subtraction, an inclusive compare."""
    a, b = np.float32(a), np.float32(b)
    if not (valid(a) and valid(b)):
        return False
    return bool(np.abs(np.float32(a - b)) <= np.float32(max_diff))


def component_sizes(disp, max_diff):
    """sizes [H,W] uint32: the pixel count of each pixel's 4-connected component, 0 for invalid pixels."""
    disp = np.asarray(disp, np.float32)
    H, W = disp.shape
    sizes = np.zeros((H, W), np.uint32)
    seen = ~valid(disp)
    for h0 in range(H):
        for w0 in range(W):
            if seen[h0, w0]:
                continue
            seen[h0, w0] = True
            stack, members = [(h0, w0)], []
            while stack:
                h, w = stack.pop()
                members.append((h, w))
                for y, x in ((h - 1, w), (h + 1, w), (h, w - 1), (h, w + 1)):
                    if 0 <= y < H and 0 <= x < W and not seen[y, x] and linked(disp[h, w], disp[y, x], max_diff):
                        seen[y, x] = True
                        stack.append((y, x))
            for h, w in members:
                sizes[h, w] = len(members)
    return sizes


def component_sizes_equal_values(disp):
    """A second, independent statement for max_diff = 0, where "linked" is "equal value": scipy labels the 4-connected
    regions of each value's mask.  (Also what the maps too large for the flood fill are checked against.)"""
    from scipy import ndimage
    disp = np.asarray(disp, np.float32)
    ok = valid(disp)
    sizes = np.zeros(disp.shape, np.uint32)
    for v in np.unique(disp[ok]):                      # -0.0 == 0.0: one value
        labels, n = ndimage.label(ok & (disp == v))   # the default structure: 4-neighbours, no diagonals
        if n:
            counts = np.bincount(labels.reshape(-1), minlength=n + 1)
            counts[0] = 0
            sizes += counts[labels].astype(np.uint32)
    return sizes


def random_map(H, W, seed, levels=3, step=1.0, bad=0.10):
    """Values from a few levels `step` apart, so that components are large; a share `bad` of the pixels holds NaN, +inf,
    -inf, -1 (invalid) or -0.0 (valid)."""
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, levels, (H, W)) * step).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0], np.float32)
    count = int(round(H * W * bad))
    m.reshape(-1)[rng.choice(H * W, count, replace=False)] = odd[np.arange(count) % len(odd)]   # every kind from 5 on
    return m


def speckle_filter(disp, min_size, max_diff=1.0, sizes=None):
    """-> (out, sizes): disp where the component has at least min_size pixels, +inf elsewhere."""
    disp = np.asarray(disp, np.float32)
    sizes = component_sizes(disp, max_diff) if sizes is None else sizes
    return np.where(sizes >= np.uint32(min_size), disp, INF).astype(np.float32), sizes


def semi_dense(disp, rule, status=None, planes=None, plane_names=()):
    """sparse = speckle_filter(select(map)); `rule` has require_match, thresholds and speckle (None or (min_size,
    max_diff)) - a stereo_device.SemiDenseRule, or anything shaped like one."""
    out = select(disp, status, planes, plane_names, rule.thresholds, rule.require_match)
    if rule.speckle is not None:
        out = speckle_filter(out, rule.speckle[0], rule.speckle[1])[0]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
