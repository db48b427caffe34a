"""NumPy restatement of mccnn_evaluate_quantiles and mccnn_evaluate_quantiles_pooled, written from the definition in
include/mccnn.h - no code shared with the kernels.

keys(disp, gt, mask) -> {"all": uint32 keys, "nonocc": uint32 keys}: the bit patterns of fabsf(disp - gt) over each
region's scored pixels.  quantiles(disp, gt, mask, ppm) -> {region: dict(n_scored, rank=[...], value=[uint32 bits])}: the
keys sorted, the integer rank formula, the canonical NaN for an empty region.  Pool models the device-resident histogram:
np.bincount(keys >> 16) accumulated over maps, and the pooled pick.  loop() is the definition pixel by pixel in plain
Python, for tiny maps.
"""
import math

import numpy as np

REGIONS = ("all", "nonocc")
NAN_BITS = 0x7fc00000
POOL_BINS = 65536
MIDDLEBURY = (500000, 900000, 950000, 990000)


def rank_of(q_ppm, n):
    """max(ceil(q_ppm * n / 10^6) - 1, 0) in exact integers (Python's are unbounded)."""
    return (int(q_ppm) * int(n) + 999999) // 1000000 - 1 if n > 0 else 0


def keys(disp, gt, mask=None):
    disp = np.asarray(disp, np.float32).reshape(-1)
    gt = np.asarray(gt, np.float32).reshape(-1)
    in_all = np.isfinite(gt)
    regions = {"all": in_all,
               "nonocc": in_all if mask is None else in_all & (np.asarray(mask, np.uint8).reshape(-1) == 255)}
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(disp) & ~(disp < np.float32(0))
        err = np.abs(disp - gt)                       # float32 subtraction
    assert err.dtype == np.float32
    return {name: err[regions[name] & valid].view(np.uint32).copy() for name in REGIONS}


def select(sorted_keys, ppm):
    """dict(n_scored, rank, value) of ascending uint32 keys."""
    n = int(sorted_keys.size)
    ranks = [rank_of(q, n) for q in ppm]
    return dict(n_scored=n, rank=ranks, value=[int(sorted_keys[r]) if n else NAN_BITS for r in ranks])


def quantiles(disp, gt, mask, ppm):
    k = keys(disp, gt, mask)
    return {name: select(np.sort(k[name]), ppm) for name in REGIONS}


def loop(disp, gt, mask, ppm):
    """The definition pixel by pixel."""
    disp = np.asarray(disp, np.float32).reshape(-1)
    gt = np.asarray(gt, np.float32).reshape(-1)
    m = None if mask is None else np.asarray(mask, np.uint8).reshape(-1)
    out = {}
    for name in REGIONS:
        ks = []
        for i in range(disp.size):
            g, d = float(gt[i]), float(disp[i])
            if not math.isfinite(g) or not (name == "all" or m is None or int(m[i]) == 255):
                continue
            if not math.isfinite(d) or d < 0:
                continue
            with np.errstate(over="ignore"):
                err = np.float32(abs(np.float32(disp[i] - gt[i])))
            ks.append(int(np.array([err], np.float32).view(np.uint32)[0]))
        ks.sort()
        n = len(ks)
        ranks = [max(-(-(q * n) // 1000000) - 1, 0) for q in ppm]       # ceil by floor division of the negation
        out[name] = dict(n_scored=n, rank=ranks if n else [0] * len(ppm), value=[ks[r] if n else NAN_BITS for r in ranks])
    return out


class Pool(object):
    """pool[2][65536] of counts: region, then key >> 16."""

    def __init__(self):
        self.counts = np.zeros((2, POOL_BINS), np.uint64)

    def add(self, disp, gt, mask=None):
        k = keys(disp, gt, mask)
        for r, name in enumerate(REGIONS):
            self.counts[r] += np.bincount(k[name] >> 16, minlength=POOL_BINS).astype(np.uint64)
        return self

    def pick(self, ppm):
        """The pooled values: the bits bin << 16 of the bin that holds each rank of the pooled counts."""
        out = {}
        for r, name in enumerate(REGIONS):
            cum = np.cumsum(self.counts[r], dtype=np.uint64)            # exact integers
            n = int(cum[-1])
            ranks = [rank_of(q, n) for q in ppm]
            value = [int(np.searchsorted(cum, np.uint64(rk), side="right")) << 16 if n else NAN_BITS
                     for rk in ranks]                                    # first bin whose running count exceeds the rank
            out[name] = dict(n_scored=n, rank=ranks, value=value)
        return out


def same(got, want):
    """n_scored, every rank and every value's bits; `got` may carry more entries than compared."""
    for name in REGIONS:
        g, w = got[name], want[name]
        k = len(w["rank"])
        if int(g["n_scored"]) != w["n_scored"] or [int(x) for x in g["rank"][:k]] != w["rank"] \
                or [int(x) for x in g["value"][:k]] != w["value"]:
            return False
    return True


def bits_of(x):
    """A float (or None: the empty region) as the uint32 bits of its float32."""
    return NAN_BITS if x is None else int(np.array([x], np.float32).view(np.uint32)[0])


def make_case(H, W, seed, with_mask=True, d_max=64.0, sigma=1.5):
    """Seeded maps in the manner of evaluation_reference.make_case: gt with +inf, -inf, NaN and finite values; disp with
    NaN, +-inf, -1, -0.0 and errors spread over many octaves (a normal error times a log-uniform scale), so that every
    digit of the key varies; masks drawn from {0, 1, 128, 254, 255}."""
    rng = np.random.default_rng(seed)
    n = H * W
    gt = (np.round(rng.uniform(0.0, d_max, n) * 4) / 4).astype(np.float32)
    scale = np.exp2(rng.uniform(-12.0, 2.0, n))
    disp = np.abs(gt + rng.normal(0.0, sigma, n) * scale).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=n, p=[0.1, 0.05, 0.15, 0.05, 0.65])
    gt[rng.random(n) < 0.08] = np.inf
    gt[rng.random(n) < 0.02] = -np.inf
    gt[rng.random(n) < 0.02] = np.nan
    for value, p in ((np.nan, 0.02), (np.inf, 0.01), (-np.inf, 0.01), (-1.0, 0.04), (-0.0, 0.01)):
        disp[rng.random(n) < p] = value
    return disp.reshape(H, W), gt.reshape(H, W), (mask.reshape(H, W) if with_mask else None)
