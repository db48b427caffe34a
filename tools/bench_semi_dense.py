#!/usr/bin/env python3
"""The semi-dense maps' cost (run under `timeout -k 10 300`): writes one JSON object to profiles/semi_dense.json.

    python tools/bench_semi_dense.py [--out profiles/semi_dense.json] [--rounds 5] [--iters 2000] [--pair-iters 100]

At 750 x 500 and 2880 x 1988:
  - mccnn_semi_dense_select (status + one plane) and mccnn_speckle_filter (min_size 20, max_diff 1, out and sizes) alone,
    beside mccnn_median 5x5 on the same map, alternating leg by leg in one process (HIP events around `iters` launches;
    the median and the lowest leg of `rounds`).  The maps: the final map of a matched synthetic pair behind the `lr`
    selection (the real case), and the two adversarial ones - a constant map (ONE component: every count goes to one
    word) and the serpentine corridor (one component with the longest label chains).
  - the captured 750 x 500 x 256 pair (match_graph) with semi_dense="lr,speckle:20:1" and without, alternating in the same
    way, and of a second matcher without the option: what two captures of one pair differ by.
The one condition: the single-component map must not cost an order of magnitude more than the real map of its size.
"""
import argparse
import json
import os
import statistics
import sys

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


def serpentine(H, W):
    disp = np.zeros((H, W), np.float32)
    disp[1::2] = -1.0
    walls = np.arange(1, H, 2)
    disp[walls, np.where((walls // 2) % 2 == 0, W - 1, 0)] = 0.0
    return disp


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_dense.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pair-iters", type=int, default=100)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters,
                  rule=RULE, shapes={})
    for H, W, D in SHAPES:
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
        l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        keep = {}
        m = sd.StereoMatcher(net, on_saturation="ignore", confidence=("mmn",), semi_dense=RULE)
        dense, planes, sparse = m.match(l, r, D, keep=keep)
        status, selected = keep["status"].clone(), keep["semi_dense_selected"].clone()
        density = float(torch.isfinite(sparse).float().mean())
        del keep, m
        torch.cuda.empty_cache()
        maps = dict(real=selected, constant=torch.zeros_like(dense), serpentine=torch.from_numpy(serpentine(H, W)).cuda())
        out, sizes = torch.empty_like(dense), torch.empty((H, W), dtype=torch.int32, device="cuda")
        scratch = sd.speckle_scratch(H, W, "cuda")
        variants = {"mccnn_median_5x5": lambda: sd.median(dense, 5, 5, out=out),
                    "select_lr_mmn": lambda: sd.semi_dense_select(dense, status, planes, ("mmn",), {"mmn": 0.5}, True, out=out)}
        for name, disp in maps.items():
            variants["speckle_" + name] = (
                lambda disp=disp: sd.speckle_filter(disp, 20, 1.0, out=out, sizes=sizes, scratch=scratch))
        iters = args.iters if H * W < 1 << 20 else max(50, args.iters // 10)
        kernel = alternate(variants, args.rounds, iters)
        median_ms = kernel["mccnn_median_5x5"]["median_ms"]
        for v in kernel.values():
            v["times_median_5x5"] = v["median_ms"] / median_ms
        entry = dict(kernel=kernel, density_of_the_real_map=density,
                     constant_over_real=kernel["speckle_constant"]["median_ms"] / kernel["speckle_real"]["median_ms"],
                     serpentine_over_real=kernel["speckle_serpentine"]["median_ms"] / kernel["speckle_real"]["median_ms"])
        print("%dx%d  median %.4f ms, select %.4f ms, speckle real %.4f / constant %.4f / serpentine %.4f ms" % (
            W, H, median_ms, kernel["select_lr_mmn"]["median_ms"], kernel["speckle_real"]["median_ms"],
            kernel["speckle_constant"]["median_ms"], kernel["speckle_serpentine"]["median_ms"]), flush=True)
        del maps, variants
        torch.cuda.empty_cache()
        if (H, W, D) == SHAPES[0]:
            plain = sd.StereoMatcher(net, on_saturation="ignore")
            semi = sd.StereoMatcher(net, on_saturation="ignore", semi_dense=RULE)
            again = sd.StereoMatcher(net, on_saturation="ignore")
            pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_semi_dense": lambda: semi.match_graph(l, r, D),
                              "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
            assert torch.equal(plain.match_graph(l, r, D), semi.match_graph(l, r, D)[0])
            del plain, semi, again
            torch.cuda.empty_cache()
            pair["added_ms"] = pair["pair_semi_dense"]["median_ms"] - pair["pair"]["median_ms"]
            pair["capture_spread_ms"] = abs(pair["pair_again"]["median_ms"] - pair["pair"]["median_ms"])
            entry["captured_pair"] = pair
            print("%dx%dx%d  pair %.3f -> %.3f ms (a second plain matcher: %.3f)" % (
                W, H, D, pair["pair"]["median_ms"], pair["pair_semi_dense"]["median_ms"], pair["pair_again"]["median_ms"]),
                flush=True)
        result["shapes"]["%dx%d" % (W, H)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
