#!/usr/bin/env python3
"""What measuring a pair's row offset and matching along it cost (run under `timeout -k 10 300`): writes one JSON
object to profiles/vertical_offset.json.

    python tools/bench_vertical_offset.py [--out profiles/vertical_offset.json] [--rounds 5] [--iters 300] [--pair-iters 50]

At 750 x 500 x 256 and 1242 x 375 x 228, on the features of a synthetic pair whose right image sits two rows low:
  - mccnn_cost_volume_hwd (MCCNN_CV_EXACT), time T0: the yardstick, taken in the same process in the same run;
  - mccnn_vertical_profile at (max_offset, row_step) = (4, 8) and (8, 8), mccnn_vertical_offset_select on the votes of
    (4, 8), and mccnn_cost_volume_offset_hwd along the measured offset at vertical_range 0 and 1 (2 and 6 product sets),
    each as a multiple of T0 - the launches alternate leg by leg (HIP events around `iters` launches; the median and
    the lowest leg of `rounds`), every launch on the same features and into the same buffers;
  - the captured pair (match_graph) of a matcher with vertical_offset="auto" and of one without, alternating in the same
    way, and of a second matcher without the option: two captures of one pair differ by more than a small kernel takes.
The expectations reported beside the figures (product sets x T0 x 1.25): the offset volume at range 0 within 2.5 T0, the
profile at (4, 8) within (9 / 8) x 1.25 T0.
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
PROFILES = ((4, 8), (8, 8))                        # (max_offset, row_step)
RANGES = (0, 1)
MARGIN = 1.25
DY = 2


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_offset.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--pair-iters", type=int, default=50)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters,
                  margin=MARGIN, rows_low=DY, shapes={})
    for H, W, D in SHAPES:
        l8, r8, _ = synthetic.make_scene_u8(H, W, D, 100)
        r8 = r8[[max(0, h - DY) for h in range(H)]]             # the right image DY rows low, its edge row repeated
        l = torch.from_numpy(synthetic.standardize(l8)[:, :, 0].copy()).cuda()
        r = torch.from_numpy(synthetic.standardize(r8)[:, :, 0].copy()).cuda()
        fl, fr = (t.clone() for t in net.features_pair_hwc_split(l, r))
        out = tuple(torch.zeros((H, W, sd.hwd_pitch(D)), dtype=torch.float32, device="cuda") for _ in range(2))
        votes = {p: sd.vertical_profile(fl, fr, D, p[0], p[1]) for p in PROFILES}
        offset, totals = sd.vertical_offset_select(votes[PROFILES[0]], PROFILES[0][0])
        measured = sd.vertical_record(offset.cpu().numpy(), totals.cpu().numpy())
        variants = {"mccnn_cost_volume_hwd": lambda: sd.cost_volume_hwd(fl, fr, D, out=out)}
        for p in PROFILES:
            variants["profile_%d_%d" % p] = lambda p=p: sd.vertical_profile(fl, fr, D, p[0], p[1], out=votes[p])
        variants["select"] = lambda: sd.vertical_offset_select(votes[PROFILES[0]], PROFILES[0][0], out=(offset, totals))
        for rng in RANGES:
            variants["offset_range_%d" % rng] = lambda rng=rng: sd.cost_volume_offset_hwd(fl, fr, D, offset, rng, out=out)
        kernel = alternate(variants, args.rounds, args.iters)
        t0 = kernel["mccnn_cost_volume_hwd"]["median_ms"]
        for name, v in kernel.items():
            v["times_T0"] = v["median_ms"] / t0
        for rng in RANGES:
            v = kernel["offset_range_%d" % rng]
            v["product_sets"] = 2 * (2 * rng + 1)
            v["times_T0_per_product_set"] = v["times_T0"] / v["product_sets"]
        expected = dict(offset_range_0_within_2p5_T0=kernel["offset_range_0"]["times_T0"] <= 2 * MARGIN,
                        profile_4_8_within_9_8ths_x_1p25_T0=kernel["profile_4_8"]["times_T0"] <= 9.0 / 8.0 * MARGIN)
        del fl, fr, out, votes
        torch.cuda.empty_cache()
        plain = sd.StereoMatcher(net, on_saturation="ignore")
        auto = sd.StereoMatcher(net, on_saturation="ignore", extras=dict(vertical_offset="auto"))
        again = sd.StereoMatcher(net, on_saturation="ignore")
        pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_auto": lambda: auto.match_graph(l, r, D),
                          "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
        pair["report"] = auto.vertical_report(H, W, D)
        del plain, auto, again
        torch.cuda.empty_cache()
        pair["added_ms"] = pair["pair_auto"]["median_ms"] - pair["pair"]["median_ms"]
        result["shapes"]["%dx%dx%d" % (W, H, D)] = dict(T0_ms=t0, measured=measured, kernel=kernel, expected=expected,
                                                        captured_pair=pair)
        print("%dx%dx%d  T0 %.4f ms; profile (4, 8) %.2f x, (8, 8) %.2f x, select %.4f ms, offset volume range 0 %.2f x, "
              "range 1 %.2f x T0; measured offset %d (share %.3f); pair %.3f -> %.3f ms with 'auto' (a second plain "
              "matcher: %.3f)" % (
                  W, H, D, t0, kernel["profile_4_8"]["times_T0"], kernel["profile_8_8"]["times_T0"],
                  kernel["select"]["median_ms"], kernel["offset_range_0"]["times_T0"], kernel["offset_range_1"]["times_T0"],
                  measured["offset"], measured["share"], pair["pair"]["median_ms"], pair["pair_auto"]["median_ms"],
                  pair["pair_again"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
