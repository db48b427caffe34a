"""Readers of tests/golden/route_*.npz (made by tests/golden/gen_route_golden.py from the reference's own runs), shared by
test_reference_routes_cpu.py and test_reference_routes_gpu.py.  Loaded once; the arrays are handed out read-only."""
import functools
import glob
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIRS = dict(right=(0, 1), left=(0, -1), up=(-1, 0), bottom=(1, 0))       # pf:194-208, in SGM_average's order
SGM_CLASSES = (5, 130, 192, 256, 257, 512, 513, 768, 769, 1024)
POST_WINDOWS = ((5, 5), (3, 7))
POST_BILATERAL = ((6, 2), (1, 0.5))


@functools.lru_cache(maxsize=None)
def family(prefix):
    """[(file name without .npz, {key: read-only array})] of route_<prefix>*.npz, sorted by name."""
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, "route_%s*.npz" % prefix)))
    assert paths, "route fixtures missing - run tests/golden/gen_route_golden.py in the dev container"
    out = []
    for p in paths:
        g = dict(np.load(p))
        for v in g.values():
            v.setflags(write=False)
        out.append((os.path.basename(p)[:-4], g))
    return out


def names(prefix):
    return [n for n, _ in family(prefix)]


def fixture(name):
    return dict(family(name.split("_")[1]))[name]


def sgm_sides(g):
    """The sides a route_sgm_* file holds ("l", "r"; the penalty-class fixture has one file per side)."""
    return [s for s in "lr" if "vol_" + s in g]


def sgm_route(D):
    """csrc/sgm_route.h's sgm_route(D, far_volume = false), restated: (groups, full, disparities per lane)."""
    dp = (D + 3) & ~3
    ng = (dp + 255) // 256
    vpl = 3 if 128 < D <= 192 and dp % 3 == 0 else 4
    return ng, D == 64 * vpl * ng, vpl


# the ten near classes: one to four groups, tail-masked and full, and the two three-per-lane forms
SGM_NEAR_CLASSES = {(1, False, 4), (1, False, 3), (1, True, 3), (1, True, 4), (2, False, 4), (2, True, 4), (3, False, 4),
                    (3, True, 4), (4, False, 4), (4, True, 4)}


def cbca_cases(g):
    return [(int(d), int(i)) for d, i in g["cases"]]
