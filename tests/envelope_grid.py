"""The shapes at the edges of check_envelope (H >= 1, 2 <= D <= 1024, D <= W - 2) that the whole-pair tests share:
test_envelope_edges_cpu.py (the grid itself and the oracle on it), test_envelope_edges_gpu.py (StereoMatcher) and
test_envelope_edges_dropin_gpu.py (process_functional).  Every value sits on a kernel's edge:

    H = 1 .. 6       rows below the 5x5 median and bilateral windows and below the row batches; SGM columns shorter than
                     every pipeline depth (6 to 24 steps in flight)
    H = 13, 14, 15   either side of the arm limit at distance 14
    H = 28, 29, 30   either side of a full vertical arm (2 * 14 + 1 rows)
    D = W - 2        the longest border recurrence of the cost volume (every (W, D) of the grid but (20, 2))
    D = 2, 3, 5, 17, 19, 39   a padded pitch
    D = 64 / 65, 129, 256 / 257, 1024   tile and group boundaries, the three-per-lane SGM route, one against two chunks
                     (the WTA fused into the last aggregation launch against its own launch)
    W = 19, 20, 21 and 66, 67   either side of the patch and tile widths
"""
HEIGHTS = (1, 2, 3, 4, 5, 6, 13, 14, 15, 28, 29, 30)
WIDTH_DISPARITIES = ((4, 2), (5, 2), (5, 3), (6, 4), (7, 5), (19, 17), (20, 2), (21, 19), (41, 39), (66, 64), (67, 65))
EXTRAS = ((1, 258, 256), (2, 259, 257), (1, 1026, 1024), (3, 131, 129), (300, 4, 2), (65, 5, 3))

FULL = tuple((H, W, D) for H in HEIGHTS for W, D in WIDTH_DISPARITIES) + EXTRAS

REDUCED_HEIGHTS = (1, 5, 14, 29)
REDUCED_WIDTH_DISPARITIES = ((4, 2), (7, 5), (21, 19), (67, 65))
REDUCED = (tuple((H, W, D) for H in REDUCED_HEIGHTS for W, D in REDUCED_WIDTH_DISPARITIES)
           + ((1, 258, 256), (2, 259, 257), (3, 131, 129)))

# the aggregation distances of the grid: match.py's default and one of the long-arm kernels
DISTANCES = (14, 28)


def shapes_of_height(H):
    """The eleven shapes of the full grid with H rows."""
    return tuple(s for s in FULL[:len(HEIGHTS) * len(WIDTH_DISPARITIES)] if s[0] == H)


def name(shape):
    """'WxHxD', the form every failure message carries."""
    return "%dx%dx%d" % (shape[1], shape[0], shape[2])


def make_pair(shape):
    """The grid's pair of a shape: (left, right) standardised float32 [H,W,1]."""
    import synthetic
    H, W, D = shape
    return synthetic.make_pair(H, W, D, seed=H + W + D)[:2]


def make_scene_u8(shape):
    """The bytes of the grid's pair: (left_u8, right_u8) uint8 [H,W]."""
    import synthetic
    H, W, D = shape
    return synthetic.make_scene_u8(H, W, D, seed=H + W + D)[:2]


def unit_features(shape, seed=None):
    """Seeded random unit features (left, right) float32 [H,W,64] for the oracle's chain behind the network."""
    import numpy as np
    H, W, D = shape
    rng = np.random.default_rng(H + W + D if seed is None else seed)
    out = []
    for _ in range(2):
        f = rng.standard_normal((H, W, 64))
        out.append((f / np.sqrt((f * f).sum(-1, keepdims=True))).astype(np.float32))
    return out
