#!/usr/bin/env python3
"""The vertical search's cost (run under `timeout -k 10 300`): writes one JSON object to profiles/vertical.json.

    python tools/bench_vertical.py [--out profiles/vertical.json] [--rounds 5] [--iters 300] [--pair-iters 50]

At 750 x 500 x 256 and 1242 x 375 x 228, on the features of a synthetic pair:
  - mccnn_cost_volume_hwd (MCCNN_CV_EXACT), time T0: the yardstick, taken in the same process in the same run;
  - mccnn_cost_volume_vertical_hwd at vertical_range 0, 1 and 2, each as a multiple of T0 and of its product count
    (1, 6 and 10 product sets: 2 (2r + 1) for r > 0) - the launches alternate leg by leg (HIP events around `iters`
    launches; the median and the lowest leg of `rounds`), every launch on the same features and into the same volumes;
  - the captured pair (match_graph) of a matcher with vertical_range=1 and of one without, alternating in the same way,
    and of a second matcher without the option: two captures of one pair differ by more than a small kernel takes.
The margins reported: range 0 within 1.25 x T0, range 1 within 1.25 x 5 T0 (the expectation by product count).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

import torch  # noqa: E402

import _hipabi as hip  # noqa: E402
import stereo_device as sd  # noqa: E402
import synthetic  # noqa: E402
import tf_checkpoint  # noqa: E402
from model import NET  # noqa: E402

SHAPES = ((500, 750, 256), (375, 1242, 228))       # (H, W, D)
RANGES = (0, 1, 2)
MARGIN = 1.25


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical.json"))
    ap.add_argument("--rounds", type=int, default=5)
    # a leg is a timed window of 0.2 s and more even for the plain kernel; the range-2 legs take seconds
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--pair-iters", type=int, default=50)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters,
                  margin=MARGIN, shapes={})
    for H, W, D in SHAPES:
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
        l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        fl, fr = (t.clone() for t in net.features_pair_hwc_split(l, r))
        out = tuple(torch.zeros((H, W, sd.hwd_pitch(D)), dtype=torch.float32, device="cuda") for _ in range(2))
        variants = {"mccnn_cost_volume_hwd": lambda: sd.cost_volume_hwd(fl, fr, D, out=out)}
        for rng in RANGES:
            variants["vertical_range_%d" % rng] = lambda rng=rng: sd.cost_volume_vertical_hwd(fl, fr, D, rng, out=out)
        kernel = alternate(variants, args.rounds, args.iters)
        t0 = kernel["mccnn_cost_volume_hwd"]["median_ms"]
        for rng in RANGES:
            v = kernel["vertical_range_%d" % rng]
            v["product_sets"] = 1 if rng == 0 else 2 * (2 * rng + 1)
            v["times_T0"] = v["median_ms"] / t0
            v["times_T0_per_product_set"] = v["times_T0"] / v["product_sets"]
        within = dict(range_0_within_1p25_T0=kernel["vertical_range_0"]["times_T0"] <= MARGIN,
                      range_1_within_1p25_x_5_T0=kernel["vertical_range_1"]["times_T0"] <= MARGIN * 5)
        del fl, fr, out
        torch.cuda.empty_cache()
        plain = sd.StereoMatcher(net, on_saturation="ignore")
        vert = sd.StereoMatcher(net, on_saturation="ignore", extras=dict(vertical_range=1))
        again = sd.StereoMatcher(net, on_saturation="ignore")
        pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_vertical_1": lambda: vert.match_graph(l, r, D),
                          "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
        del plain, vert, again
        torch.cuda.empty_cache()
        pair["added_ms"] = pair["pair_vertical_1"]["median_ms"] - pair["pair"]["median_ms"]
        result["shapes"]["%dx%dx%d" % (W, H, D)] = dict(T0_ms=t0, kernel=kernel, within=within, captured_pair=pair)
        print("%dx%dx%d  T0 %.4f ms; range 0 %.2f x, range 1 %.2f x, range 2 %.2f x T0; pair %.3f -> %.3f ms with range 1 "
              "(a second plain matcher: %.3f)" % (
                  W, H, D, t0, kernel["vertical_range_0"]["times_T0"], kernel["vertical_range_1"]["times_T0"],
                  kernel["vertical_range_2"]["times_T0"], pair["pair"]["median_ms"], pair["pair_vertical_1"]["median_ms"],
                  pair["pair_again"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
