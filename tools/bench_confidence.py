#!/usr/bin/env python3
"""The confidence measures' cost (run under `timeout -k 10 300`): writes one JSON object to profiles/confidence.json.

    python tools/bench_confidence.py [--out profiles/confidence.json] [--rounds 5] [--iters 8000] [--pair-iters 100]

At 750 x 500 x 256 and 1242 x 375 x 228, on the final left volume and right map of a matched synthetic pair:
  - mccnn_confidence_hwd alone, for each single measure and for all four, beside mccnn_wta_hwd on the same volume - the
    launches alternate leg by leg in one process (HIP events around `iters` launches; the median and the lowest leg of
    `rounds`), with the algorithmic GB/s of the one read of the volume - the SAME buffer read again and again, launch after
    launch, so whatever of it the last-level cache keeps is not fetched from HBM: not a cold-HBM figure; and all four on a volume of signed zeros, where
    every pixel's runner-up is looked up a second time (the kernel's worst case);
  - the captured pair (match_graph) of a matcher with confidence= all four and of one without, alternating in the same way,
    and of a second matcher without the option: two captures of one pair differ by more than the kernel takes.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence.json"))
    ap.add_argument("--rounds", type=int, default=5)
    # a leg is a timed window of 0.7 s and more (8000 launches of 0.08 .. 0.18 ms; 100 pairs of 8 .. 11 ms): shorter
    # windows measure the clock and the scheduler as much as the kernel
    ap.add_argument("--iters", type=int, default=8000)
    ap.add_argument("--pair-iters", type=int, default=100)
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters,
                  shapes={})
    for H, W, D in SHAPES:
        L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
        l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        keep = {}
        sd.StereoMatcher(net, on_saturation="ignore").match(l, r, D, keep=keep)
        vol = sd.dhw_to_hwd(keep["cbca2"][0])
        right = keep["wta"][1].clone()
        del keep
        torch.cuda.empty_cache()
        disp = torch.empty((H, W), dtype=torch.float32, device="cuda")
        planes = torch.empty((4, H, W), dtype=torch.float32, device="cuda")
        variants = {"mccnn_wta_hwd": lambda: sd.wta_hwd(vol, D, out=disp)}
        for names in [(n,) for n in sd.CONFIDENCE_MEASURES] + [sd.CONFIDENCE_MEASURES]:
            variants["confidence_" + "+".join(names)] = (
                lambda names=names: sd.confidence_hwd(vol, D, right, names, out=planes[:len(names)]))
        # the worst case of the runner-up's second look (a runner-up that compares equal to zero is fetched again by index:
        # the pixel's row is read a second time): a volume of zeros of both signs, where every pixel takes it
        zeros = torch.where(torch.rand_like(vol) < 0.5, torch.zeros_like(vol), -torch.zeros_like(vol))
        variants["confidence_all_four_on_zeros"] = (
            lambda: sd.confidence_hwd(zeros, D, right, sd.CONFIDENCE_MEASURES, out=planes))
        kernel = alternate(variants, args.rounds, args.iters)
        del zeros
        read_bytes = 4.0 * H * W * sd.hwd_pitch(D)
        for v in kernel.values():
            v["read_GBs"] = read_bytes / (v["median_ms"] * 1e6)
        wta_ms = kernel["mccnn_wta_hwd"]["median_ms"]
        for name, v in kernel.items():
            v["times_wta_hwd"] = v["median_ms"] / wta_ms
        del vol
        torch.cuda.empty_cache()
        plain = sd.StereoMatcher(net, on_saturation="ignore")
        conf = sd.StereoMatcher(net, on_saturation="ignore", confidence=sd.CONFIDENCE_MEASURES)
        # (a second matcher without the option: what two captures of the same pair differ by, the yardstick for the row
        # beside it)
        again = sd.StereoMatcher(net, on_saturation="ignore")
        pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_confidence": lambda: conf.match_graph(l, r, D),
                          "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
        assert torch.equal(plain.match_graph(l, r, D), conf.match_graph(l, r, D)[0])
        del plain, conf, again
        torch.cuda.empty_cache()
        pair["added_ms"] = pair["pair_confidence"]["median_ms"] - pair["pair"]["median_ms"]
        result["shapes"]["%dx%dx%d" % (W, H, D)] = dict(volume_read_bytes=read_bytes, kernel=kernel, captured_pair=pair)
        print("%dx%dx%d  wta_hwd %.4f ms, all four %.4f ms (%.2f x), pair %.3f -> %.3f ms (a second plain matcher: %.3f)" % (
            W, H, D, wta_ms, kernel["confidence_msm+mmn+cur+lrc"]["median_ms"],
            kernel["confidence_msm+mmn+cur+lrc"]["times_wta_hwd"], pair["pair"]["median_ms"],
            pair["pair_confidence"]["median_ms"], pair["pair_again"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
