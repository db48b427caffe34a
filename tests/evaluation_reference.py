"""NumPy restatement of mccnn_evaluate, written from the definition in include/mccnn.h - no code shared with the kernel.

evaluate(disp, gt, mask, thresholds) -> {"all": {...}, "nonocc": {...}} with n_valid, n_invalid, n_bad (list), sum_abs,
sum_sq; the sums follow the defined order: chunks of 1024 consecutive pixels, zero padded, the stride-halving tree inside
a chunk, the chunk partials added in ascending order from +0.0 (a Python loop: np.sum adds pairwise).
evaluate_loop is the per-pixel definition of the counts (and of the terms) in plain Python, for tiny maps.
accumulate(old, new) restates accumulate != 0: counts added, each sum old + this call's total.
"""
import functools
import math
import struct

import numpy as np

CHUNK = 1024
REGIONS = ("all", "nonocc")


def tree_sum(terms):
    """terms: float64, flat, in pixel order -> the bit-defined sum."""
    n = terms.size
    chunks = -(-n // CHUNK)
    x = np.zeros(chunks * CHUNK, np.float64)
    x[:n] = terms
    x = x.reshape(-1, CHUNK)
    s = CHUNK // 2
    while s >= 1:
        x = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return float(functools.reduce(lambda acc, p: acc + p, (float(p) for p in x[:, 0]), 0.0))


def evaluate(disp, gt, mask, thresholds):
    disp = np.asarray(disp, np.float32).reshape(-1)
    gt = np.asarray(gt, np.float32).reshape(-1)
    thresholds = [np.float32(t) for t in thresholds]
    in_all = np.isfinite(gt)
    regions = {"all": in_all,
               "nonocc": in_all if mask is None else in_all & (np.asarray(mask, np.uint8).reshape(-1) == 255)}
    with np.errstate(invalid="ignore", over="ignore"):
        invalid = ~np.isfinite(disp) | (disp < np.float32(0))
        err = np.abs(disp - gt)                       # float32 subtraction
        assert err.dtype == np.float32
        a = err.astype(np.float64)
        q = a * a
    out = {}
    for name in REGIONS:
        reg = regions[name]
        scored = reg & ~invalid
        with np.errstate(invalid="ignore"):
            n_bad = [int(np.count_nonzero(scored & (err > t))) for t in thresholds]
        out[name] = dict(n_valid=int(np.count_nonzero(reg)), n_invalid=int(np.count_nonzero(reg & invalid)), n_bad=n_bad,
                         sum_abs=tree_sum(np.where(scored, a, 0.0)), sum_sq=tree_sum(np.where(scored, q, 0.0)))
    return out


def evaluate_loop(disp, gt, mask, thresholds):
    """The definition pixel by pixel: the counts, and the per-pixel terms (for the sums of maps of one chunk at most)."""
    disp = np.asarray(disp, np.float32).reshape(-1)
    gt = np.asarray(gt, np.float32).reshape(-1)
    m = None if mask is None else np.asarray(mask, np.uint8).reshape(-1)
    out = {}
    for name in REGIONS:
        r = dict(n_valid=0, n_invalid=0, n_bad=[0] * len(thresholds), terms_abs=[], terms_sq=[])
        for i in range(disp.size):
            g, d = float(gt[i]), float(disp[i])
            inside = math.isfinite(g) and (name == "all" or m is None or int(m[i]) == 255)
            a = q = 0.0
            if inside:
                r["n_valid"] += 1
                if not math.isfinite(d) or d < 0:
                    r["n_invalid"] += 1
                else:
                    err = np.float32(abs(np.float32(disp[i] - gt[i])))
                    for k, t in enumerate(thresholds):
                        if err > np.float32(t):
                            r["n_bad"][k] += 1
                    a = float(err)
                    q = float(err) * float(err)
            r["terms_abs"].append(a)
            r["terms_sq"].append(q)
        out[name] = r
    return out


def accumulate(old, new):
    out = {}
    for name in REGIONS:
        o, n = old[name], new[name]
        out[name] = dict(n_valid=o["n_valid"] + n["n_valid"], n_invalid=o["n_invalid"] + n["n_invalid"],
                         n_bad=[x + y for x, y in zip(o["n_bad"], n["n_bad"])],
                         sum_abs=o["sum_abs"] + n["sum_abs"], sum_sq=o["sum_sq"] + n["sum_sq"])
    return out


def bits(x):
    """A float64 as its uint64 bit pattern."""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same(got, want):
    """Counts as integers, sums as bit patterns; `got` may carry more thresholds' worth of keys than compared."""
    for name in REGIONS:
        g, w = got[name], want[name]
        if (g["n_valid"], g["n_invalid"], list(g["n_bad"])) != (w["n_valid"], w["n_invalid"], list(w["n_bad"])):
            return False
        if bits(g["sum_abs"]) != bits(w["sum_abs"]) or bits(g["sum_sq"]) != bits(w["sum_sq"]):
            return False
    return True


def make_case(H, W, seed, thresholds=(0.5, 1.0, 2.0, 4.0), with_mask=True, d_max=64.0):
    """Seeded maps that carry every special content the definition names (each present once the map has >= 16 pixels):
    gt with +inf, -inf, NaN and finite values; disp with NaN, +-inf, -1, -0.0, values above and below gt, and errors
    exactly equal to a threshold (must not count); masks drawn from {0, 1, 128, 254, 255}."""
    rng = np.random.default_rng(seed)
    n = H * W
    gt = rng.uniform(0.0, d_max, n).astype(np.float32)
    # quarter-pixel ground truth keeps gt +- threshold exact in float32, so "err == threshold" really is equality
    gt = (np.round(gt * 4) / 4).astype(np.float32)
    disp = (gt + rng.normal(0.0, 1.5, n)).astype(np.float32)
    disp = np.where(disp < 0, -disp, disp).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=n, p=[0.1, 0.05, 0.15, 0.05, 0.65])
    # a share of errors exactly on a threshold
    on = rng.random(n) < 0.1
    t = np.asarray(thresholds, np.float32)[rng.integers(0, len(thresholds), n)]
    sign = np.where(rng.random(n) < 0.5, np.float32(1), np.float32(-1)).astype(np.float32)
    exact = (gt + sign * t).astype(np.float32)
    ok = on & (exact >= 0)
    disp = np.where(ok, exact, disp).astype(np.float32)
    # random specials ...
    gt[rng.random(n) < 0.08] = np.inf
    gt[rng.random(n) < 0.02] = -np.inf
    gt[rng.random(n) < 0.02] = np.nan
    for value, p in ((np.nan, 0.02), (np.inf, 0.01), (-np.inf, 0.01), (-1.0, 0.04), (-0.0, 0.01)):
        disp[rng.random(n) < p] = value
    # ... and one of each at a seeded position once there is room
    if n >= 16:
        pos = iter(rng.permutation(n)[:16])
        for v in (np.inf, -np.inf, np.nan):
            gt[next(pos)] = v
        for v in (np.nan, np.inf, -np.inf, -1.0, -0.0):
            i = next(pos)
            disp[i], gt[i], mask[i] = v, np.float32(3.25), 255
        for d in (10.0 + thresholds[0], 14.5, 7.0):          # err == a threshold, above gt, below gt
            i = next(pos)
            gt[i], disp[i], mask[i] = np.float32(10.0), np.float32(d), 255
    return (disp.reshape(H, W), gt.reshape(H, W), mask.reshape(H, W) if with_mask else None)
