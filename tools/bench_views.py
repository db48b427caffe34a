#!/usr/bin/env python3
"""What views="both" costs (run once, under `timeout -k 10 600`): writes one JSON object to profiles/views.json.

    python tools/bench_views.py [--out profiles/views.json] [--rounds 3] [--leg-seconds 0.6] [--pair-iters 100]

At 750 x 500 x 256 and 1242 x 375 x 228, on the winner-take-all maps and final volumes of a matched synthetic pair:
  (a) every mirrored kernel beside its left twin on the same maps - mccnn_lr_status / _right, mccnn_interpolate(_ex) /
      _right in the modes (4, 0) and (16, 1), mccnn_confidence_hwd / _right_hwd with all four measures - the launches
      alternating leg by leg in one process (HIP events around a leg; the median and the lowest leg of `rounds`).  A leg
      is as many launches as fill `leg-seconds` (counted in a calibration leg): shorter windows measure the clock and the
      scheduler as much as the kernel.  The operands are read again and again, so whatever the last-level cache keeps is
      not fetched from HBM: not cold-HBM figures.  ratio = right median / left median;
  (b) the captured pair (match_graph) of a views="both" matcher, of a views="left" one and of a second views="left" one
      (what two captures of one pair differ by: the yardstick for the row beside it), alternating in the same way.
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


def leg(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, rounds, iters_of):
    """{name: fn} -> {name: dict(median_ms, min_ms, legs_ms, iters)}: one warm-up leg each, then `rounds` rounds in which
    every variant runs one leg, in turn.  iters_of(name, warm_ms) -> the launches of a leg."""
    iters = {}
    for name, fn in variants.items():
        leg(fn, 20)
        iters[name] = iters_of(name, leg(fn, 200))
    legs = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            legs[name].append(leg(fn, iters[name]))
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), legs_ms=v, iters=iters[name])
            for name, v in legs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-seconds", type=float, default=0.6)
    ap.add_argument("--pair-iters", type=int, default=100)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, leg_seconds=args.leg_seconds,
                  pair_iters=args.pair_iters, shapes={})

    def kernel_iters(_name, warm_ms):
        return max(200, int(args.leg_seconds * 1000.0 / max(warm_ms, 1e-4)))

    for H, W, D in SHAPES:
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
        l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        keep = {}
        sd.StereoMatcher(net, on_saturation="ignore").match(l, r, D, keep=keep)
        vol_l, vol_r = sd.dhw_to_hwd(keep["cbca2"][0]), sd.dhw_to_hwd(keep["cbca2"][1])
        dl, dr = keep["wta"][0].clone(), keep["wta"][1].clone()
        del keep
        torch.cuda.empty_cache()
        st_l, st_r = sd.lr_status(dl, dr, D), sd.lr_status_right(dr, dl, D)
        out = torch.empty((H, W), dtype=torch.float32, device="cuda")
        status = torch.empty((H, W), dtype=torch.int32, device="cuda")
        planes = torch.empty((4, H, W), dtype=torch.float32, device="cuda")
        variants = {
            "lr_status/left": lambda: sd.lr_status(dl, dr, D, out=status),
            "lr_status/right": lambda: sd.lr_status_right(dr, dl, D, out=status),
            "interpolate_4_0/left": lambda: sd.interpolate(dl, st_l, out=out),
            "interpolate_4_0/right": lambda: sd.interpolate_right(dr, st_r, out=out),
            "interpolate_16_1/left": lambda: sd.interpolate(dl, st_l, out=out, directions=16, occlusion_from_left=True),
            "interpolate_16_1/right": lambda: sd.interpolate_right(dr, st_r, out=out, directions=16,
                                                                   occlusion_from_right=True),
            "confidence_all_four/left": lambda: sd.confidence_hwd(vol_l, D, dr, sd.CONFIDENCE_MEASURES, out=planes),
            "confidence_all_four/right": lambda: sd.confidence_right_hwd(vol_r, D, dl, sd.CONFIDENCE_MEASURES, out=planes),
        }
        kernel = alternate(variants, args.rounds, kernel_iters)
        ratios = {name[:-len("/right")]: kernel[name]["median_ms"] / kernel[name[:-len("/right")] + "/left"]["median_ms"]
                  for name in kernel if name.endswith("/right")}
        states = dict(left=[float((st_l == k).float().mean()) for k in (0, 1, 2)],
                      right=[float((st_r == k).float().mean()) for k in (0, 1, 2)])
        del vol_l, vol_r
        torch.cuda.empty_cache()
        left = sd.StereoMatcher(net, on_saturation="ignore")
        both = sd.StereoMatcher(net, on_saturation="ignore", views="both")
        again = sd.StereoMatcher(net, on_saturation="ignore")
        pair = alternate({"pair_left": lambda: left.match_graph(l, r, D), "pair_both": lambda: both.match_graph(l, r, D),
                          "pair_left_again": lambda: again.match_graph(l, r, D)}, args.rounds,
                         lambda _name, _ms: args.pair_iters)
        assert torch.equal(left.match_graph(l, r, D), both.match_graph(l, r, D)[0])
        del left, both, again
        torch.cuda.empty_cache()
        pair["added_ms"] = pair["pair_both"]["median_ms"] - pair["pair_left"]["median_ms"]
        pair["ratio"] = pair["pair_both"]["median_ms"] / pair["pair_left"]["median_ms"]
        pair["capture_to_capture_ms"] = abs(pair["pair_left_again"]["median_ms"] - pair["pair_left"]["median_ms"])
        result["shapes"]["%dx%dx%d" % (W, H, D)] = dict(
            right_volume_store_bytes=4.0 * H * W * sd.hwd_pitch(D), status_shares_0_1_2=states, kernel=kernel,
            right_over_left=ratios, captured_pair=pair)
        print("%dx%dx%d  right/left: %s; pair %.3f -> %.3f ms (x %.3f; a second left matcher: %.3f)" % (
            W, H, D, ", ".join("%s %.2f" % kv for kv in sorted(ratios.items())), pair["pair_left"]["median_ms"],
            pair["pair_both"]["median_ms"], pair["ratio"], pair["pair_left_again"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
