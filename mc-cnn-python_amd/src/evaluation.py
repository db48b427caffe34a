"""Scoring of disparity maps against Middlebury ground truth: the host side of mccnn_evaluate (csrc/evaluate.hip), and
against KITTI's through mccnn_evaluate_kitti (csrc/kitti.hip; KittiEvaluator, data set layouts: datasets.py).

The counting and the sums happen on the device (stereo_device.evaluate: bad-pixel counts, invalid pixels and the float64
error sums of the regions `all` and `nonocc`, defined to the bit in include/mccnn.h); this module turns the 192 bytes of a
result into the figures of the Middlebury tables, finds the ground truth beside a left image, and keeps the per-pair
results and the running total of a list on the device until somebody asks for them.

    bad[t]  = 100 * (n_bad[t] + n_invalid) / n_valid        per cent of the region's pixels off by more than t, the
                                                            pixels without a disparity counted as bad
    invalid = 100 * n_invalid / n_valid
    avgerr  = sum_abs / (n_valid - n_invalid)               over the pixels that have a disparity
    rms     = sqrt(sum_sq / (n_valid - n_invalid))
A figure whose denominator is zero is None (JSON null).

On request (Evaluator(quantiles=...), match.py --eval_quantiles) also the error quantiles of the Middlebury tables
(A50, A90, A95, A99, ...): per map the exact nearest-rank quantiles of the error over each region's scored pixels
(stereo_device.evaluate_quantiles, csrc/evaluate_quantiles.hip), for a list the quantiles of a device-resident histogram
of the error's top 16 bits.  A quantile of a region without scored pixels is None.
"""
import ctypes
import json
import math
import os

import numpy as np

import util

GT_SUFFIX = "disp0GT.pfm"        # beside im0.png, like match.py's left_gt_suffix
MASK_SUFFIX = "mask0nocc.png"    # 255 non-occluded, 128 occluded, 0 unknown
LEFT_SUFFIX = "im0.png"
RIGHT_GT_SUFFIX = "disp1GT.pfm"      # the right view's, match.py --views both
RIGHT_MASK_SUFFIX = "mask1nocc.png"
DEFAULT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
REGIONS = ("all", "nonocc")
RESULT_BYTES = 192


def parse_thresholds(text):
    """'0.5,1,2,4' -> (0.5, 1.0, 2.0, 4.0); 1 to 8 values, none of them NaN."""
    values = tuple(float(t) for t in str(text).split(",") if t.strip())
    if not 1 <= len(values) <= 8 or any(math.isnan(v) for v in values):
        raise ValueError("expected 1 to 8 comma-separated thresholds, got %r" % (text,))
    return values


def parse_kitti_thresholds(text):
    """'3:0.05,2' -> ((3.0, 0.05), (2.0, 0.0)): 1 to 8 abs[:rel] items for mccnn_evaluate_kitti - a pixel is bad when its
    error exceeds abs pixels and rel times the true disparity.  Neither part may be NaN or negative, and the abs parts
    are distinct: they name the figures in the JSON files."""
    pairs = []
    for item in str(text).split(","):
        if not item.strip():
            continue
        parts = item.split(":")
        if len(parts) > 2:
            raise ValueError("expected abs[:rel], got %r" % (item,))
        pairs.append((float(parts[0]), float(parts[1]) if len(parts) == 2 else 0.0))
    if not 1 <= len(pairs) <= 8 or any(math.isnan(v) or v < 0 for pair in pairs for v in pair):
        raise ValueError("expected 1 to 8 comma-separated abs[:rel] thresholds, none NaN or negative, got %r" % (text,))
    if len(set(a for a, _ in pairs)) != len(pairs):
        raise ValueError("the abs parts name the figures and must differ, got %r" % (text,))
    return tuple(pairs)


def threshold_tag(t):
    """The name of a threshold in the JSON files and the training log: 0.5 -> '0.5', 2 -> '2.0'."""
    return repr(float(t))


QUANTILE_RESULT_BYTES = 208      # sizeof(mccnn_eval_quantiles_t)
MAX_QUANTILES = 8                # MCCNN_EVAL_MAX_QUANTILES
POOLED_QUANTILE_BITS = 16        # a list's pooled quantiles: the top 16 bits of the exact ones (include/mccnn.h)


def parse_quantiles(text):
    """'50,90,95,99.5' -> (500000, 900000, 950000, 995000): quantiles in per cent as the parts per million that
    mccnn_evaluate_quantiles takes, parsed exactly through decimal.  1 to 8 values, each with 0 < q <= 100 and at most
    four decimals; repeats and any order are allowed."""
    import decimal
    items = [t.strip() for t in str(text).split(",") if t.strip()]
    if not 1 <= len(items) <= MAX_QUANTILES:
        raise ValueError("expected 1 to %d comma-separated quantiles, got %r" % (MAX_QUANTILES, text))
    ppm = []
    for item in items:
        try:
            q = decimal.Decimal(item)
        except decimal.InvalidOperation:
            raise ValueError("%r is not a number" % (item,))
        if not q.is_finite() or not 0 < q <= 100:
            raise ValueError("a quantile is in per cent, 0 < q <= 100, got %r" % (item,))
        scaled = q * 10000
        if scaled != scaled.to_integral_value():
            raise ValueError("a quantile has at most four decimals (one part per million), got %r" % (item,))
        ppm.append(int(scaled))
    return tuple(ppm)


def quantile_percent(ppm):
    """Parts per million as the per cent a JSON file shows: 995000 -> 99.5."""
    return int(ppm) / 10000.0


def quantile_tag(ppm):
    """The name of a quantile in the JSON files, Middlebury's: 500000 -> 'A50', 995000 -> 'A99.5'."""
    import decimal
    return "A" + format((decimal.Decimal(int(ppm)) / 10000).normalize(), "f")


def _host_bytes(host_bytes):
    """A device result on the host (bytes, a NumPy array or a host tensor of any dtype) as bytes."""
    if hasattr(host_bytes, "numpy"):
        host_bytes = host_bytes.numpy()
    return bytes(host_bytes) if isinstance(host_bytes, (bytes, bytearray)) else np.ascontiguousarray(host_bytes).tobytes()


def quantile_raw(host_bytes, quantiles):
    """The 208 bytes of a mccnn_eval_quantiles_t (bytes, a NumPy array or a host tensor of any dtype) ->
    {region: dict(n_scored, quantile_rank=[...], values=[float or None, ...])}, one entry per quantile; a value is the
    float32 the device selected, None for a region without scored pixels."""
    from _hipabi import QuantileResult
    data = _host_bytes(host_bytes)
    if len(data) != QUANTILE_RESULT_BYTES or ctypes.sizeof(QuantileResult) != QUANTILE_RESULT_BYTES:
        raise ValueError("a quantile result is %d bytes, got %d" % (QUANTILE_RESULT_BYTES, len(data)))
    res = QuantileResult.from_buffer_copy(data)
    n = len(tuple(quantiles))
    out = {}
    for name in REGIONS:
        reg = getattr(res, name)
        bits = np.array([reg.value[k] for k in range(n)], dtype=np.uint32)
        scored = int(reg.n_scored)
        out[name] = dict(n_scored=scored, quantile_rank=[int(reg.rank[k]) for k in range(n)],
                         values=[float(v) if scored > 0 else None for v in bits.view(np.float32)])
    return out


class Metrics(object):
    """The figures of one mccnn_eval_t.  raw[region]: n_valid, n_invalid, n_bad (one per threshold), sum_abs, sum_sq -
    exactly what the device wrote; figures[region]: bad (dict by threshold tag), invalid, avgerr, rms.

    With `quantiles` (parts per million) and the quantile_raw() of a mccnn_eval_quantiles_t also
    figures[region]["quantiles"] = {tag: value or None}, raw[region]["n_scored"] and raw[region]["quantile_rank"];
    quantile_bits: what a pooled result says about its values' resolution.  Without them nothing is added."""

    def __init__(self, raw, thresholds, quantiles=None, quantile_values=None, quantile_bits=None):
        self.thresholds = tuple(float(t) for t in thresholds)
        self.quantiles = tuple(int(q) for q in quantiles) if quantiles else None
        self.quantile_bits = quantile_bits if self.quantiles else None
        self.raw = raw
        self.figures = {r: self._figures(raw[r]) for r in REGIONS}
        if self.quantiles:
            for r in REGIONS:
                self.raw[r] = dict(self.raw[r], n_scored=quantile_values[r]["n_scored"],
                                   quantile_rank=list(quantile_values[r]["quantile_rank"]))
                self.figures[r]["quantiles"] = {quantile_tag(q): v for q, v in zip(self.quantiles, quantile_values[r]["values"])}

    @classmethod
    def from_result(cls, host_bytes, thresholds, quantile_bytes=None, quantiles=None, quantile_bits=None):
        """host_bytes: the 192 bytes of a mccnn_eval_t (bytes, a NumPy array or a host tensor of any dtype);
        quantile_bytes: the 208 bytes of the map's mccnn_eval_quantiles_t for `quantiles`, or None."""
        from _hipabi import EvalResult
        data = _host_bytes(host_bytes)
        if len(data) != RESULT_BYTES or ctypes.sizeof(EvalResult) != RESULT_BYTES:
            raise ValueError("a result is %d bytes, got %d" % (RESULT_BYTES, len(data)))
        res = EvalResult.from_buffer_copy(data)
        n = len(tuple(thresholds))
        raw = {}
        for name in REGIONS:
            reg = getattr(res, name)
            raw[name] = dict(n_valid=int(reg.n_valid), n_invalid=int(reg.n_invalid), n_bad=[int(reg.n_bad[k]) for k in range(n)],
                             sum_abs=float(reg.sum_abs), sum_sq=float(reg.sum_sq))
        if quantile_bytes is None:
            return cls(raw, thresholds)
        return cls(raw, thresholds, quantiles, quantile_raw(quantile_bytes, quantiles), quantile_bits)

    def _figures(self, r):
        n_valid, scored = r["n_valid"], r["n_valid"] - r["n_invalid"]
        return dict(
            bad={threshold_tag(t): (100.0 * (b + r["n_invalid"]) / n_valid if n_valid > 0 else None)
                 for t, b in zip(self.thresholds, r["n_bad"])},
            invalid=100.0 * r["n_invalid"] / n_valid if n_valid > 0 else None,
            avgerr=r["sum_abs"] / scored if scored > 0 else None,
            rms=math.sqrt(r["sum_sq"] / scored) if scored > 0 else None)

    def bad(self, threshold, region):
        return self.figures[region]["bad"][threshold_tag(threshold)]

    def to_dict(self):
        """JSON-ready: the figures per region, and under "raw" the counts and the two float64 sums (Python's float repr
        round-trips, so the sums survive the file bit for bit)."""
        out = {r: self.figures[r] for r in REGIONS}
        out["raw"] = self.raw
        if self.quantile_bits is not None:
            out["quantile_bits"] = self.quantile_bits
        return out


def mean(values):
    """The mean of the values that are not None; None where there is none."""
    values = [v for v in values if v is not None]
    return sum(values) / len(values) if values else None


def mean_of(metrics):
    """Unweighted mean over pairs of every figure, per region; a pair whose figure is None does not count, and a figure
    that no pair has is None.  Pairs that carry quantiles add "quantiles": each tag averaged over the pairs that have it."""
    out = {}
    for r in REGIONS:
        figs = [m.figures[r] for m in metrics]
        tags = list(figs[0]["bad"]) if figs else []
        out[r] = dict(bad={t: mean(f["bad"][t] for f in figs) for t in tags},
                      invalid=mean(f["invalid"] for f in figs), avgerr=mean(f["avgerr"] for f in figs),
                      rms=mean(f["rms"] for f in figs))
        with_q = [f["quantiles"] for f in figs if "quantiles" in f]
        if with_q:
            out[r]["quantiles"] = {t: mean(q[t] for q in with_q if t in q) for t in with_q[0]}
    return out


def error_quantiles(disp, gt, mask=None, quantiles=(50, 90, 95, 99)):
    """NumPy in, dict out, computed on the device: disp, gt float32 [H,W], mask uint8 [H,W] or None, quantiles in per
    cent -> {region: dict(n_scored, quantiles={tag: value or None}, quantile_rank=[...])}: the exact nearest-rank
    quantiles of fabsf(disp - gt) over the region's scored pixels (include/mccnn.h: mccnn_evaluate_quantiles)."""
    import torch
    import stereo_device as sd
    device = sd.hip.require_device()
    ppm = parse_quantiles(",".join(str(q) for q in quantiles))

    def dev(a, dtype):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)

    res = sd.evaluate_quantiles(dev(disp, np.float32), dev(gt, np.float32), dev(mask, np.uint8), ppm)
    raw = quantile_raw(res.cpu(), ppm)
    return {r: dict(n_scored=raw[r]["n_scored"], quantile_rank=raw[r]["quantile_rank"],
                    quantiles={quantile_tag(q): v for q, v in zip(ppm, raw[r]["values"])}) for r in REGIONS}


def load_ground_truth(left_path, view="left"):
    """(gt float32 [H,W] with +inf where unknown, mask uint8 [H,W] or None) from disp0GT.pfm / mask0nocc.png beside the
    left image; None when there is no ground-truth file.  view="right": disp1GT.pfm / mask1nocc.png."""
    pair_dir = os.path.dirname(left_path)
    gt_name, mask_name = (GT_SUFFIX, MASK_SUFFIX) if view == "left" else (RIGHT_GT_SUFFIX, RIGHT_MASK_SUFFIX)
    gt_path = os.path.join(pair_dir, gt_name)
    if not os.path.isfile(gt_path):
        return None
    gt = np.ascontiguousarray(util.readPfm(gt_path), dtype=np.float32)
    mask_path = os.path.join(pair_dir, mask_name)
    mask = np.ascontiguousarray(util.read_gray(mask_path), dtype=np.uint8) if os.path.isfile(mask_path) else None
    if mask is not None and mask.shape != gt.shape:
        raise ValueError("%s is %s, %s is %s" % (mask_path, mask.shape, gt_path, gt.shape))
    return gt, mask


def check_shape(gt, map_shape, name):
    if tuple(gt.shape) != tuple(map_shape):
        raise ValueError("%s: the ground truth is %s, the disparity map %s (resampling is not supported)"
                         % (name, tuple(gt.shape), tuple(map_shape)))


class PairScore(object):
    """A pair's result on its way to the host: pinned bytes + the event behind the copy (with quantiles: the 208 bytes
    of the pair's mccnn_eval_quantiles_t as well, behind the same event)."""

    def __init__(self, host, done, thresholds, quantile_host=None, quantiles=None):
        self.host, self.done, self.thresholds = host, done, thresholds
        self.quantile_host, self.quantiles = quantile_host, quantiles

    def metrics(self):
        """Blocks until the bytes are on the host."""
        self.done.synchronize()
        return Metrics.from_result(self.host, self.thresholds, self.quantile_host, self.quantiles)


class Evaluator(object):
    """Per-pair results and the running total of a list, both on the device.

    score(disp, gt, mask, slot) enqueues one mccnn_evaluate on the current stream, overwriting the result buffer of
    `slot`, and the copy of its 192 bytes into pinned host memory; commit(disp, gt, mask) enqueues one accumulating
    into the total; pair() is the two together.  Nothing blocks the host until PairScore.metrics() / report().
    Scratch is private to a call in flight, so every slot has its own (a slot = one stream: match.py's pairs in flight),
    and so has the total.  The total's sums depend on the order of the additions: commits run in the order they are
    enqueued, whichever streams they are enqueued on - each waits for the event of the one before.  A caller that may
    discard a map (match.py's saturation redo) scores at once and commits only the map it keeps.

    quantiles (parts per million, parse_quantiles' result): score() also enqueues one mccnn_evaluate_quantiles into the
    slot's quantile result and the copy of its 208 bytes, commit() the pool-only call that adds the map's scored pixels
    to the list's pool (integer counts: their order does not matter), report() the pooled selection.  None: not one
    launch or buffer more."""

    def __init__(self, device=None, thresholds=DEFAULT_THRESHOLDS, slots=1, quantiles=None):
        import torch
        import stereo_device as sd
        self.torch, self.sd = torch, sd
        self.device = device if device is not None else sd.hip.require_device()
        self.thresholds = tuple(float(t) for t in thresholds)
        self.total = sd.evaluate_result(self.device)
        self.pairs = 0
        self._slot = [dict(result=sd.evaluate_result(self.device), scratch=None) for _ in range(max(1, int(slots)))]
        self._total_scratch = []       # grown, never shrunk or freed: earlier commits may still be queued on other streams
        self._last_commit = None
        self.quantiles = tuple(int(q) for q in quantiles) if quantiles else None
        if self.quantiles:
            # the selection's scratch does not depend on the map's size: one per slot, one for the commits (which run
            # one behind the other)
            for st in self._slot:
                st.update(quantile_result=sd.evaluate_quantiles_result(self.device),
                          quantile_scratch=sd.evaluate_quantiles_scratch(1, 1, self.device))
            self.pool = sd.evaluate_quantiles_pool(self.device)
            self._pool_scratch = sd.evaluate_quantiles_scratch(1, 1, self.device)

    def describe(self):
        """What the JSON files say beside the figures."""
        return dict(quantiles=[quantile_percent(q) for q in self.quantiles]) if self.quantiles else {}

    # the three places that name the entry point (KittiEvaluator puts mccnn_evaluate_kitti there)
    def _scratch_bytes(self, H, W):
        return int(self.sd.hip.load().mccnn_evaluate_scratch_bytes(H, W))

    def _new_scratch(self, H, W):
        return self.sd.evaluate_scratch(H, W, self.device)

    def _evaluate(self, disp, gt, mask, **kw):
        self.sd.evaluate(disp, gt, mask, self.thresholds, **kw)

    def _scratch(self, have, H, W):
        """`have` if it serves an H x W map, else a new scratch."""
        need = self._scratch_bytes(H, W)
        if have is not None and have.numel() * have.element_size() >= need:
            return have
        return self._new_scratch(H, W)

    def score(self, disp, gt, mask=None, slot=0):
        torch, sd = self.torch, self.sd
        st = self._slot[slot]
        st["scratch"] = self._scratch(st["scratch"], disp.shape[0], disp.shape[1])
        self._evaluate(disp, gt, mask, out=st["result"], scratch=st["scratch"])
        host = torch.empty((RESULT_BYTES // 8,), dtype=torch.int64, pin_memory=True)
        host.copy_(st["result"], non_blocking=True)
        quantile_host = None
        if self.quantiles:
            sd.evaluate_quantiles(disp, gt, mask, self.quantiles, out=st["quantile_result"], scratch=st["quantile_scratch"])
            quantile_host = torch.empty((QUANTILE_RESULT_BYTES // 8,), dtype=torch.int64, pin_memory=True)
            quantile_host.copy_(st["quantile_result"], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return PairScore(host, done, self.thresholds, quantile_host, self.quantiles)

    def commit(self, disp, gt, mask=None):
        torch, sd = self.torch, self.sd
        stream = torch.cuda.current_stream()
        if self._last_commit is not None:
            stream.wait_event(self._last_commit)
        scratch = self._scratch(self._total_scratch[-1] if self._total_scratch else None, disp.shape[0], disp.shape[1])
        if not self._total_scratch or scratch is not self._total_scratch[-1]:
            self._total_scratch.append(scratch)
        self._evaluate(disp, gt, mask, out=self.total, accumulate=True, scratch=scratch)
        if self.quantiles:
            sd.evaluate_quantiles(disp, gt, mask, self.quantiles, out=False, pool=self.pool, scratch=self._pool_scratch)
        self._last_commit = torch.cuda.Event()
        self._last_commit.record(stream)
        self.pairs += 1

    def pair(self, disp, gt, mask=None, slot=0):
        """Two calls on the current stream: the pair's own result (overwritten) and the running total (accumulated)."""
        score = self.score(disp, gt, mask, slot)
        self.commit(disp, gt, mask)
        return score

    def report(self):
        """The pooled Metrics of everything committed so far (synchronises)."""
        if self._last_commit is not None:
            self._last_commit.synchronize()
        if not self.quantiles:
            return Metrics.from_result(self.total.cpu(), self.thresholds)
        pooled = self.sd.evaluate_quantiles_pooled(self.pool, self.quantiles)
        return Metrics.from_result(self.total.cpu(), self.thresholds, pooled.cpu(), self.quantiles, POOLED_QUANTILE_BITS)


class KittiEvaluator(Evaluator):
    """The same bookkeeping on mccnn_evaluate_kitti: `gt` is the uint16 disp_occ plane and `mask` the uint16 disp_noc
    plane (or None) as the kit stores them, thresholds are (abs, rel) pairs, interpolate fills the pixels without a
    disparity as the kit does before they are scored.  Metrics names a figure by the abs part of its pair."""

    def __init__(self, device=None, thresholds=((3.0, 0.05),), slots=1, interpolate=False, quantiles=None):
        if quantiles:
            raise ValueError("KittiEvaluator: KITTI's protocol has no error quantiles (and the 16-bit truth has no "
                             "quantile entry point)")
        self.pairs_thresholds = tuple((float(a), float(r)) for a, r in thresholds)
        self.interpolate = bool(interpolate)
        Evaluator.__init__(self, device, tuple(a for a, _ in self.pairs_thresholds), slots)

    def _scratch_bytes(self, H, W):
        return int(self.sd.hip.load().mccnn_evaluate_kitti_scratch_bytes(H, W, 1 if self.interpolate else 0))

    def _new_scratch(self, H, W):
        return self.sd.evaluate_kitti_scratch(H, W, self.device, self.interpolate)

    def _evaluate(self, disp, gt, mask, **kw):
        self.sd.evaluate_kitti(disp, gt, mask, self.pairs_thresholds, interpolate=self.interpolate, **kw)

    def describe(self):
        """What the JSON files say beside the figures."""
        return dict(rel_thresholds=[r for _, r in self.pairs_thresholds], interpolate=self.interpolate)


# ---- a score for confidence measures: the sparsification curve ---------------------------------------------------------
# Take the n pixels of region `all`, ordered by confidence descending (a NaN confidence counts as -inf; ties by ascending
# pixel index h*W + w: a stable sort, so that ties cannot move the curve).  B(k) = the bad pixels among the first k.
#     auc         = (1/n) sum_{k=1..n} B(k) / k
#     auc_optimal = (1/n) sum_{k=n-e+1..n} (k - (n-e)) / k,  e = B(n): the curve of the ordering that puts every bad pixel last
# both float64.  A measure is the better the closer its auc is to auc_optimal; bad_rate = e / n is where every curve ends.
def _f32(x):
    """A Python scalar with the value float32 gives it: compared with (or multiplied into) a float32 tensor it behaves as
    the float32 number, whichever precision the comparison runs in."""
    return float(np.float32(x))


def bad_and_region(disp, gt, threshold=1.0):
    """Middlebury: (bad, region) bool [H,W] device tensors for a float32 map and ground truth.  region: gt finite (`all`
    of mccnn_evaluate); bad: the estimate invalid (not finite, or < 0) or fabsf(disp - gt) > threshold in float32."""
    import torch
    region = torch.isfinite(gt)
    invalid = ~torch.isfinite(disp) | (disp < 0)
    err = (disp - gt).abs()
    # (thresholds are Python scalars rounded to float32: a device tensor made from a host scalar is a blocking copy, which
    # would make the calling thread wait for the pair just enqueued on this stream)
    return (invalid | (err > _f32(threshold))) & region, region


def bad_and_region_kitti(disp, gt_occ_u16, abs_thr=3.0, rel_thr=0.05):
    """KITTI (gt_occ_u16: the kit's 16-bit codes, uint16 or a wider integer tensor): region: gt_occ != 0 (`all` of
    mccnn_evaluate_kitti), truth g = code / 256; bad: the estimate invalid, or err > abs_thr and err > rel_thr * g,
    float32 throughout."""
    import torch
    if gt_occ_u16.dtype == torch.uint16:
        code = gt_occ_u16.view(torch.int16).to(torch.int32) & 0xFFFF
    else:
        code = gt_occ_u16.to(torch.int32)
    region = code != 0
    g = code.to(torch.float32) / 256.0
    invalid = ~torch.isfinite(disp) | (disp < 0)
    err = (disp - g).abs()
    return (invalid | ((err > _f32(abs_thr)) & (err > g * _f32(rel_thr)))) & region, region


def sparsification(confidence, bad, region):
    """confidence: float32 [K,H,W] planes; bad, region: bool [H,W] -> float64 device tensor [3 + K]: n, e, auc_optimal and
    the K values of auc.  torch on the current stream; no host synchronisation and no data-dependent shape: a pixel
    outside the region gets key -inf and weight 0, ranks are the running count of the weights, n stays on the device
    (n = 0 gives NaN for the three figures)."""
    import torch
    K = confidence.shape[0]
    region = region.reshape(-1)
    bad = (bad.reshape(-1) & region).to(torch.float64)
    weight = region.to(torch.float64)
    key = confidence.reshape(K, -1)
    key = key.masked_fill(torch.isnan(key) | ~region[None, :], float("-inf")) + 0.0  # (+ 0.0: -0.0 ties with +0.0)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    w = weight[order]
    rank = torch.cumsum(w, dim=1)                                                    # k at every in-region pixel
    run = torch.cumsum(bad[order], dim=1)                                            # B(k)
    terms = torch.where(w > 0, run / rank.clamp(min=1.0), torch.zeros_like(run))
    n, e = weight.sum(), bad.sum()
    auc = terms.sum(dim=1) / n
    k = torch.arange(1, region.numel() + 1, dtype=torch.float64, device=confidence.device)
    first = n - e
    optimal = torch.where((k > first) & (k <= n), (k - first) / k, torch.zeros_like(k)).sum() / n
    return torch.cat([torch.stack([n, e, optimal]), auc])


def sparsification_figures(values, names, threshold):
    """The JSON entry of a pair from the host copy of sparsification()'s result."""
    values = [float(v) for v in values]
    n, e = int(values[0]), int(values[1])
    return dict(threshold=threshold, n=n, bad_rate=(e / n if n > 0 else None), auc_optimal=values[2] if n > 0 else None,
                auc={name: (values[3 + i] if n > 0 else None) for i, name in enumerate(names)})


class SparsificationScore(object):
    """A pair's sparsification figures on their way to the host, like PairScore: pinned float64 values + the event behind
    the copy."""

    def __init__(self, host, done, names, threshold):
        self.host, self.done, self.names, self.threshold = host, done, names, threshold

    def figures(self):
        """Blocks until the values are on the host."""
        self.done.synchronize()
        return sparsification_figures(self.host.numpy(), self.names, self.threshold)


class Sparsifier(object):
    """match.py --evaluate --confidence: scores the confidence planes of a map against its ground truth.  threshold: a
    float T (Middlebury: bad when err > T) or an (abs, rel) pair (KITTI: gt is the uint16 disp_occ plane)."""

    def __init__(self, names, threshold):
        self.names = tuple(names)
        self.kitti = isinstance(threshold, (tuple, list))
        self.threshold = [float(t) for t in threshold] if self.kitti else float(threshold)

    def score(self, disp, planes, gt):
        """Enqueued on the current stream behind the map and its planes, outside any captured graph; the 3 + K float64
        values cross to pinned host memory where the pair's 192-byte result does.  Nothing blocks the host."""
        import torch
        if self.kitti:
            bad, region = bad_and_region_kitti(disp, gt, *self.threshold)
        else:
            bad, region = bad_and_region(disp, gt, self.threshold)
        values = sparsification(planes, bad, region)
        host = torch.empty((3 + len(self.names),), dtype=torch.float64, pin_memory=True)
        host.copy_(values, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return SparsificationScore(host, done, self.names, self.threshold)


def mean_sparsification(figures):
    """Unweighted mean over the scored pairs of bad_rate, auc_optimal and every measure's auc; a pair whose figure is
    None (an empty region) does not count."""
    names = list(figures[0]["auc"]) if figures else []
    return dict(threshold=figures[0]["threshold"] if figures else None, pairs=len(figures),
                bad_rate=mean(f["bad_rate"] for f in figures), auc_optimal=mean(f["auc_optimal"] for f in figures),
                auc={n: mean(f["auc"][n] for f in figures) for n in names})


def semi_dense_block(metrics, rule=None):
    """The "semi_dense" block of a sparse map (match.py --semi_dense --evaluate) from the Metrics of mccnn_evaluate on it -
    a dropped pixel (+inf) counts as invalid there: Metrics.to_dict(), `density` per region = 100 (n_valid - n_invalid) /
    n_valid, `bad_of_scored` per region and threshold = 100 n_bad / (n_valid - n_invalid), None when nothing is scored;
    and the rule's text where given."""
    out = dict(metrics.to_dict())
    out["density"], out["bad_of_scored"] = {}, {}
    for r in REGIONS:
        raw = metrics.raw[r]
        n_valid, scored = raw["n_valid"], raw["n_valid"] - raw["n_invalid"]
        out["density"][r] = 100.0 * scored / n_valid if n_valid > 0 else None
        out["bad_of_scored"][r] = {threshold_tag(t): (100.0 * b / scored if scored > 0 else None)
                                   for t, b in zip(metrics.thresholds, raw["n_bad"])}
    if rule is not None:
        out["rule"] = rule
    return out


def semi_dense_mean(metrics):
    """mean_of() over the sparse maps of a list, with the unweighted means of `density` and `bad_of_scored` besides."""
    out = mean_of(metrics)
    blocks = [semi_dense_block(m) for m in metrics]
    tags = list(blocks[0]["bad_of_scored"][REGIONS[0]]) if blocks else []
    out["density"] = {r: mean(b["density"][r] for b in blocks) for r in REGIONS}
    out["bad_of_scored"] = {r: {t: mean(b["bad_of_scored"][r][t] for b in blocks) for t in tags} for r in REGIONS}
    return out


def write_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


class _ViewBook(object):
    """One view's part of a ListReport: the scored maps by list index, the pairs skipped for this view, and the
    evaluator whose device total pools the view over the list."""

    def __init__(self, evaluator, semi_evaluator=None, rule=None):
        self.evaluator = evaluator
        self.scored = {}         # index -> (Metrics, the map's sparsification figures or None: match.py --confidence)
        self.skipped = {}        # index -> name
        # match.py --semi_dense: the evaluator whose device total pools the view's SPARSE maps, the rule's text, and
        # index -> Metrics of the pair's sparse map
        self.semi_evaluator, self.rule, self.semi = semi_evaluator, rule, {}

    def block(self, index):
        """The view's fields in a pair's entry: the metrics, with --confidence also "sparsification" (without it no
        such key, so that the files keep their bytes).  None for a pair whose map of this view was not scored."""
        if index not in self.scored:
            return None
        metrics, figures = self.scored[index]
        semi = dict(semi_dense=semi_dense_block(self.semi[index], self.rule)) if index in self.semi else {}
        return dict(metrics.to_dict(), **(dict(sparsification=figures) if figures is not None else {}), **semi)

    def totals(self):
        """The view's fields in the list's file: the device total, the means over the scored pairs, the skipped."""
        order = sorted(self.scored)
        means = mean_of([self.scored[i][0] for i in order])
        figures = [self.scored[i][1] for i in order if self.scored[i][1] is not None]
        if figures:
            means["sparsification"] = mean_sparsification(figures)
        semi = {}
        if self.semi_evaluator is not None:
            semi = dict(semi_dense=dict(rule=self.rule, pooled=semi_dense_block(self.semi_evaluator.report()),
                                        mean=semi_dense_mean([self.semi[i] for i in order if i in self.semi])))
        return dict(pooled=self.evaluator.report().to_dict(), mean=means,
                    skipped=[self.skipped[i] for i in sorted(self.skipped)], **semi)


class ListReport(object):
    """What match.py --evaluate collects over a list: per-pair metrics by list index (set by the thread that writes the
    pair's files), the skipped pairs, and at the end the file with the pooled totals of the device accumulator.

    One book per view.  The right one (match.py --views both) has a second evaluator, whose total pools the RIGHT maps
    against disp1GT.pfm; a pair's right view is scored where its left view is and it has that file, and listed as skipped
    for the right view otherwise.  Without a right evaluator no file has a "right" key.
    semi (match.py --semi_dense): (the rule's text, an evaluator for the left view's sparse maps, one for the right view's
    or None); every view's block and totals then carry "semi_dense".  Without it no file has that key."""

    def __init__(self, evaluator, right_evaluator=None, semi=None):
        self.evaluator, self.right_evaluator = evaluator, right_evaluator
        self.extra = evaluator.describe() if hasattr(evaluator, "describe") else {}     # more keys in every file
        rule, semi_left, semi_right = semi if semi is not None else (None, None, None)
        self.semi_evaluators = (semi_left, semi_right) if semi is not None else None
        self.left, self.right = _ViewBook(evaluator, semi_left, rule), _ViewBook(right_evaluator, semi_right, rule)
        self.names = {}          # index -> name, of the pairs whose left map was scored

    def _entry(self, index):
        right = self.right.block(index)
        return dict(self.left.block(index), pair=self.names[index], **(dict(right=right) if right is not None else {}))

    def pair(self, index, name, metrics, path=None, sparsification=None, right=None, semi_dense=None):
        """right: None or dict(metrics=Metrics, sparsification=figures or None); semi_dense: None or the Metrics of the
        sparse maps of the views that were scored, the left one first.  A second call replaces the first."""
        self.names[index] = name
        self.left.scored[index] = (metrics, sparsification)
        for book, m in zip((self.left, self.right), tuple(semi_dense or ()) + (None, None)):
            if m is not None:
                book.semi[index] = m
            else:
                book.semi.pop(index, None)
        if right is not None:
            self.right.scored[index] = (right["metrics"], right.get("sparsification"))
        else:
            self.right.scored.pop(index, None)
        if path is not None:
            write_json(path, dict(self._entry(index), thresholds=list(metrics.thresholds), **self.extra))

    def skip(self, index, name):
        self.left.skipped[index] = name

    def skip_right(self, index, name):
        self.right.skipped[index] = name

    def write(self, path):
        right = dict(right=self.right.totals()) if self.right_evaluator is not None else {}
        write_json(path, dict(self.left.totals(), thresholds=list(self.evaluator.thresholds),
                              pairs=[dict(self._entry(i), index=i) for i in sorted(self.names)], **self.extra, **right))


class Scored(object):
    """A pair on its way through a ListScorer: which pair, the device ground truth (gt, mask or None) of every view that
    is scored (left first), and per view the (PairScore, SparsificationScore or None) of the maps kept so far."""

    def __init__(self, index, name, truths):
        self.index, self.name, self.truths, self.scores = index, name, truths, None
        self.semi = None         # --semi_dense: per view the PairScore of the sparse map kept so far


class ListScorer(object):
    """match.py --evaluate, for every loop over a list: which views of a pair are scored, in which order the calls are
    enqueued, what the running totals take and what the report is told.

        scored = scorer.begin(index, name, truth, truth_right)    None: no ground truth, the pair is listed as skipped
        scorer.score(scored, result, slot)                        behind the results on the pair's stream; again with the
                                                                  result of a repeated pair (the saturation redo)
        scorer.commit(scored, result)                             once, in list order, with the result that is kept
        scorer.publish(scored, json_path)                         by whoever writes the pair's files

    result: the pair's PairResult (pair_result.py) on the device - the map that is scored, the planes or None, the sparse
    map (--semi_dense) or None.  score() and commit() enqueue on the current stream and never block the host; publish()
    waits for the scores' own events.  views="both": maps are [2,H,W] and planes [2,K,H,W], and the report's right
    evaluator scores the right map of a pair with right-view ground truth.  sparsifier (--confidence): scores a map's
    planes behind its evaluation."""

    def __init__(self, report, sparsifier=None, views="left"):
        self.report, self.sparsifier, self.both = report, sparsifier, views == "both"
        self.evaluators = (report.evaluator, report.right_evaluator)

    def begin(self, index, name, truth, truth_right=None):
        """truth, truth_right: (gt, mask or None) on the device, or None.  The right view is scored where the left one
        is: right-view ground truth without the left view's is ignored."""
        if truth is None or not self.both:
            truth_right = None
        if truth is None:
            self.report.skip(index, name)
        if self.both and truth_right is None:
            self.report.skip_right(index, name)
        if truth is None:
            return None
        return Scored(index, name, [truth] if truth_right is None else [truth, truth_right])

    def _views(self, scored, result):
        """(view number, that view of the result, gt, mask) of every view of the pair that is scored, the left one first."""
        for v, (gt, mask) in enumerate(scored.truths):
            yield v, result.view(v, self.both), gt, mask

    def score(self, scored, result, slot):
        """Per view the evaluation, then (--confidence) the sparsification; replaces what the record holds.  The views'
        sparse maps (--semi_dense) are scored behind them by evaluators of their own."""
        scored.scores = [(self.evaluators[v].score(r.map, gt, mask, slot),
                          self.sparsifier.score(r.map, r.planes, gt) if self.sparsifier is not None else None)
                         for v, r, gt, mask in self._views(scored, result)]
        if result.sparse is not None:
            scored.semi = [self.report.semi_evaluators[v].score(r.sparse, gt, mask, slot)
                           for v, r, gt, mask in self._views(scored, result)]

    def commit(self, scored, result):
        """The result that is kept into the running totals (Evaluator.commit keeps the commits in call order)."""
        for v, r, gt, mask in self._views(scored, result):
            self.evaluators[v].commit(r.map, gt, mask)
        if result.sparse is not None:
            for v, r, gt, mask in self._views(scored, result):
                self.report.semi_evaluators[v].commit(r.sparse, gt, mask)

    def publish(self, scored, json_path):
        """The pair's entry of the report and its evalMCCNN.json, from the scores the record holds now."""
        views = [dict(metrics=s.metrics(), sparsification=a.figures() if a is not None else None) for s, a in scored.scores]
        semi = dict(semi_dense=[s.metrics() for s in scored.semi]) if scored.semi is not None else {}
        self.report.pair(scored.index, scored.name, views[0]["metrics"], json_path,
                         sparsification=views[0]["sparsification"], right=views[1] if len(views) > 1 else None, **semi)


