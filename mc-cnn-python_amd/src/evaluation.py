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


class Metrics(object):
    """The figures of one mccnn_eval_t.  raw[region]: n_valid, n_invalid, n_bad (one per threshold), sum_abs, sum_sq -
    exactly what the device wrote; figures[region]: bad (dict by threshold tag), invalid, avgerr, rms."""

    def __init__(self, raw, thresholds):
        self.thresholds = tuple(float(t) for t in thresholds)
        self.raw = raw
        self.figures = {r: self._figures(raw[r]) for r in REGIONS}

    @classmethod
    def from_result(cls, host_bytes, thresholds):
        """host_bytes: the 192 bytes of a mccnn_eval_t (bytes, a NumPy array or a host tensor of any dtype)."""
        from _hipabi import EvalResult
        if hasattr(host_bytes, "numpy"):
            host_bytes = host_bytes.numpy()
        data = np.ascontiguousarray(host_bytes).tobytes() if not isinstance(host_bytes, (bytes, bytearray)) else bytes(host_bytes)
        if len(data) != RESULT_BYTES or ctypes.sizeof(EvalResult) != RESULT_BYTES:
            raise ValueError("a result is %d bytes, got %d" % (RESULT_BYTES, len(data)))
        res = EvalResult.from_buffer_copy(data)
        n = len(tuple(thresholds))
        raw = {}
        for name in REGIONS:
            reg = getattr(res, name)
            raw[name] = dict(n_valid=int(reg.n_valid), n_invalid=int(reg.n_invalid), n_bad=[int(reg.n_bad[k]) for k in range(n)],
                             sum_abs=float(reg.sum_abs), sum_sq=float(reg.sum_sq))
        return cls(raw, thresholds)

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
        return out


def mean_of(metrics):
    """Unweighted mean over pairs of every figure, per region; a pair whose figure is None does not count, and a figure
    that no pair has is None."""
    def mean(values):
        values = [v for v in values if v is not None]
        return sum(values) / len(values) if values else None

    out = {}
    for r in REGIONS:
        figs = [m.figures[r] for m in metrics]
        tags = list(figs[0]["bad"]) if figs else []
        out[r] = dict(bad={t: mean(f["bad"][t] for f in figs) for t in tags},
                      invalid=mean(f["invalid"] for f in figs), avgerr=mean(f["avgerr"] for f in figs),
                      rms=mean(f["rms"] for f in figs))
    return out


def load_ground_truth(left_path):
    """(gt float32 [H,W] with +inf where unknown, mask uint8 [H,W] or None) from disp0GT.pfm / mask0nocc.png beside the
    left image; None when there is no ground-truth file."""
    pair_dir = os.path.dirname(left_path)
    gt_path = os.path.join(pair_dir, GT_SUFFIX)
    if not os.path.isfile(gt_path):
        return None
    gt = np.ascontiguousarray(util.readPfm(gt_path), dtype=np.float32)
    mask_path = os.path.join(pair_dir, MASK_SUFFIX)
    mask = np.ascontiguousarray(util.read_gray(mask_path), dtype=np.uint8) if os.path.isfile(mask_path) else None
    if mask is not None and mask.shape != gt.shape:
        raise ValueError("%s is %s, %s is %s" % (mask_path, mask.shape, gt_path, gt.shape))
    return gt, mask


def check_shape(gt, map_shape, name):
    if tuple(gt.shape) != tuple(map_shape):
        raise ValueError("%s: the ground truth is %s, the disparity map %s (resampling is not supported)"
                         % (name, tuple(gt.shape), tuple(map_shape)))


class PairScore(object):
    """A pair's result on its way to the host: pinned bytes + the event behind the copy."""

    def __init__(self, host, done, thresholds):
        self.host, self.done, self.thresholds = host, done, thresholds

    def metrics(self):
        """Blocks until the bytes are on the host."""
        self.done.synchronize()
        return Metrics.from_result(self.host, self.thresholds)


class Evaluator(object):
    """Per-pair results and the running total of a list, both on the device.

    score(disp, gt, mask, slot) enqueues one mccnn_evaluate on the current stream, overwriting the result buffer of
    `slot`, and the copy of its 192 bytes into pinned host memory; commit(disp, gt, mask) enqueues one accumulating
    into the total; pair() is the two together.  Nothing blocks the host until PairScore.metrics() / report().
    Scratch is private to a call in flight, so every slot has its own (a slot = one stream: match.py's pairs in flight),
    and so has the total.  The total's sums depend on the order of the additions: commits run in the order they are
    enqueued, whichever streams they are enqueued on - each waits for the event of the one before.  A caller that may
    discard a map (match.py's saturation redo) scores at once and commits only the map it keeps."""

    def __init__(self, device=None, thresholds=DEFAULT_THRESHOLDS, slots=1):
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
        done = torch.cuda.Event()
        done.record()
        return PairScore(host, done, self.thresholds)

    def commit(self, disp, gt, mask=None):
        torch, sd = self.torch, self.sd
        stream = torch.cuda.current_stream()
        if self._last_commit is not None:
            stream.wait_event(self._last_commit)
        scratch = self._scratch(self._total_scratch[-1] if self._total_scratch else None, disp.shape[0], disp.shape[1])
        if not self._total_scratch or scratch is not self._total_scratch[-1]:
            self._total_scratch.append(scratch)
        self._evaluate(disp, gt, mask, out=self.total, accumulate=True, scratch=scratch)
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
        return Metrics.from_result(self.total.cpu(), self.thresholds)


class KittiEvaluator(Evaluator):
    """The same bookkeeping on mccnn_evaluate_kitti: `gt` is the uint16 disp_occ plane and `mask` the uint16 disp_noc
    plane (or None) as the kit stores them, thresholds are (abs, rel) pairs, interpolate fills the pixels without a
    disparity as the kit does before they are scored.  Metrics names a figure by the abs part of its pair."""

    def __init__(self, device=None, thresholds=((3.0, 0.05),), slots=1, interpolate=False):
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


def write_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


class ListReport(object):
    """What match.py --evaluate collects over a list: per-pair metrics by list index (set by the thread that writes the
    pair's files), the skipped pairs, and at the end the file with the pooled totals of the device accumulator."""

    def __init__(self, evaluator):
        self.evaluator = evaluator
        self.extra = evaluator.describe() if hasattr(evaluator, "describe") else {}     # more keys in every file
        self.pairs = {}          # index -> (name, Metrics)
        self.skipped = {}        # index -> name

    def pair(self, index, name, metrics, path=None):
        self.pairs[index] = (name, metrics)
        if path is not None:
            write_json(path, dict(metrics.to_dict(), pair=name, thresholds=list(metrics.thresholds), **self.extra))

    def skip(self, index, name):
        self.skipped[index] = name

    def write(self, path):
        order = sorted(self.pairs)
        metrics = [self.pairs[i][1] for i in order]
        write_json(path, dict(thresholds=list(self.evaluator.thresholds),
                              pairs=[dict(self.pairs[i][1].to_dict(), pair=self.pairs[i][0], index=i) for i in order],
                              pooled=self.evaluator.report().to_dict(), mean=mean_of(metrics),
                              skipped=[self.skipped[i] for i in sorted(self.skipped)], **self.extra))
