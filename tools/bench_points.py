#!/usr/bin/env python3
"""The metric outputs' cost (run under `timeout -k 10 400`): writes one JSON object to profiles/points.json.

    python tools/bench_points.py [--out profiles/points.json] [--rounds 5] [--iters 2000] [--pair-iters 100]

At 750 x 500 and 2880 x 1988, one process, the median (and the lowest) of `rounds` legs that alternate variant by variant,
HIP events around `iters` calls:
  - mccnn_depth beside mccnn_semi_dense_select (status + one plane): both move 8 bytes per pixel;
  - the whole mccnn_reproject_points call (four launches) beside mccnn_speckle_filter (four launches) on the same map.
    The maps: the sparse map of a matched synthetic pair (the real case), an all-valid map, an all-dropped map and a 50 %
    random mask - the order of a compaction that ranks by counts must not show in its time.
  - the captured 750 x 500 x 256 pair (match_graph) with geometry=dict(depth, points) and without, alternating in the same
    way, and a second matcher without the option: what two captures of one pair differ by.  And what the matcher's choice
    for a new calibration - capture the pair again - costs: the wall time of the first match_graph under a calibration the
    matcher has not seen, beside a replay.
Expectations (written next to the figures, not gates): depth <= 1.25 x select; the cloud <= the speckle filter; all-valid
and all-dropped within 2 x the real map.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _hipabi as hip  # noqa: E402
import stereo_device as sd  # noqa: E402
import synthetic  # noqa: E402
import tf_checkpoint  # noqa: E402
from model import NET  # noqa: E402

SHAPES = ((500, 750, 256), (1988, 2880, 64))       # (H, W, D of the pair whose map is the real case)
RULE = "lr,speckle:20:1"
CALIB = (3997.684, 3997.684, 1176.728, 1011.728, 193.001, 131.111)      # a Middlebury 2014 pair's
OTHER = (1733.74, 1733.74, 792.27, 541.89, 536.62, 0.0)


def leg(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, rounds, iters):
    """{name: fn} -> {name: dict(median_ms, min_ms, legs_ms)}: one warm-up leg each, then `rounds` rounds in which every
    variant runs one leg, in turn."""
    for fn in variants.values():
        leg(fn, max(3, iters // 20))
    legs = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            legs[name].append(leg(fn, iters))
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), legs_ms=v) for name, v in legs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pair-iters", type=int, default=100)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters,
                  rule=RULE, calib=CALIB, shapes={})
    for H, W, D in SHAPES:
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
        l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        keep = {}
        m = sd.StereoMatcher(net, on_saturation="ignore", confidence=("mmn",), semi_dense=RULE)
        dense, planes, sparse = m.match(l, r, D, keep=keep)
        status = keep["status"].clone()
        density = float(torch.isfinite(sparse).float().mean())
        del keep, m
        torch.cuda.empty_cache()
        random = dense.clone()
        random[torch.from_numpy(np.random.default_rng(0).random((H, W)) < 0.5).cuda()] = float("inf")
        maps = dict(real=sparse, all_valid=torch.full_like(dense, 32.0), all_dropped=torch.full_like(dense, float("inf")),
                    random_half=random)
        out, sizes = torch.empty_like(dense), torch.empty((H, W), dtype=torch.int32, device="cuda")
        points = torch.empty((H * W, 4), dtype=torch.float32, device="cuda")
        n_points = torch.empty((1,), dtype=torch.int32, device="cuda")
        speckle, scratch = sd.speckle_scratch(H, W, "cuda"), sd.points_scratch(H, W, "cuda")
        variants = {"select_lr_mmn": lambda: sd.semi_dense_select(dense, status, planes, ("mmn",), {"mmn": 0.5}, True, out=out),
                    "depth": lambda: sd.depth(dense, CALIB, out=out)}
        for name, disp in maps.items():
            variants["speckle_" + name] = (
                lambda disp=disp: sd.speckle_filter(disp, 20, 1.0, out=out, sizes=sizes, scratch=speckle))
            variants["points_" + name] = (
                lambda disp=disp: sd.reproject(disp, CALIB, out=points, n_out=n_points, scratch=scratch))
        iters = args.iters if H * W < 1 << 20 else max(50, args.iters // 10)
        kernel = alternate(variants, args.rounds, iters)
        ms = dict((k, v["median_ms"]) for k, v in kernel.items())
        entry = dict(kernel=kernel, density_of_the_real_map=density,
                     depth_over_select=ms["depth"] / ms["select_lr_mmn"],
                     points_over_speckle=dict((k, ms["points_" + k] / ms["speckle_" + k]) for k in maps),
                     all_valid_over_real=ms["points_all_valid"] / ms["points_real"],
                     all_dropped_over_real=ms["points_all_dropped"] / ms["points_real"],
                     random_half_over_real=ms["points_random_half"] / ms["points_real"])
        print("%dx%d  select %.4f ms, depth %.4f ms; points real %.4f / all %.4f / none %.4f / half %.4f ms; speckle real "
              "%.4f ms" % (W, H, ms["select_lr_mmn"], ms["depth"], ms["points_real"], ms["points_all_valid"],
                           ms["points_all_dropped"], ms["points_random_half"], ms["speckle_real"]), flush=True)
        del maps, variants
        torch.cuda.empty_cache()
        if (H, W, D) == SHAPES[0]:
            geometry = dict(calib=CALIB, depth=True, points=True)
            plain = sd.StereoMatcher(net, on_saturation="ignore")
            metric = sd.StereoMatcher(net, on_saturation="ignore", geometry=geometry)
            again = sd.StereoMatcher(net, on_saturation="ignore")
            pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_geometry": lambda: metric.match_graph(l, r, D),
                              "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
            assert torch.equal(plain.match_graph(l, r, D), metric.match_graph(l, r, D)[0])
            pair["added_ms"] = pair["pair_geometry"]["median_ms"] - pair["pair"]["median_ms"]
            pair["capture_spread_ms"] = abs(pair["pair_again"]["median_ms"] - pair["pair"]["median_ms"])
            # a new calibration: the pair is captured again (two warm-up pairs + the capture), host wall time
            torch.cuda.synchronize()
            t0 = time.time()
            metric.set_calibration(OTHER)
            metric.match_graph(l, r, D)
            torch.cuda.synchronize()
            pair["recapture_wall_ms"] = 1e3 * (time.time() - t0)
            t0 = time.time()
            metric.set_calibration(CALIB)            # a calibration that comes back is replayed
            metric.match_graph(l, r, D)
            torch.cuda.synchronize()
            pair["replay_known_calibration_wall_ms"] = 1e3 * (time.time() - t0)
            del plain, metric, again
            torch.cuda.empty_cache()
            entry["captured_pair"] = pair
            print("%dx%dx%d  pair %.3f -> %.3f ms (a second plain matcher: %.3f); a new calibration's capture %.1f ms, a "
                  "known one's replay %.1f ms" % (W, H, D, pair["pair"]["median_ms"], pair["pair_geometry"]["median_ms"],
                                                  pair["pair_again"]["median_ms"], pair["recapture_wall_ms"],
                                                  pair["replay_known_calibration_wall_ms"]), flush=True)
        result["shapes"]["%dx%d" % (W, H)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
