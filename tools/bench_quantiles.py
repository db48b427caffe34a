#!/usr/bin/env python3
"""Times the exact error quantiles (csrc/evaluate_quantiles.hip) against mccnn_evaluate, and what match.py
--eval_quantiles costs a streamed list.

    timeout -k 10 900 python tools/bench_quantiles.py [--pairs 40] [--size 500 750 256] [--out profiles/quantiles.json]

1. The standalone calls on a 750 x 500 and a 2880 x 1988 map (mask): mccnn_evaluate_quantiles with 4 and with 8
   quantiles, the pool-only call, and mccnn_evaluate (four thresholds) on the same maps - code this tool's subject does
   not touch, the yardstick.  One process; the four calls take turns, `--legs` legs each, a leg a batch of 200 calls
   between HIP events behind 20 warm-up calls; the figure is the median over the legs, and the ratio to mccnn_evaluate is
   taken between the medians.
2. A seeded list of synthetic pairs with a ground truth and a mask beside each (tools/bench_list.py's writer,
   tools/bench_evaluate.py's truth), run in ONE process through match.main(argv) with --pipeline --evaluate, with and
   without --eval_quantiles 50,90,95,99: one untimed pass of each leg, then `--passes` timed passes, alternating.  The
   flag-less variant runs as two identical legs, so that the run's own leg-to-leg spread is on record beside the
   difference it is compared with.
Any exception ends the tool there - nothing further is started on the GPU; run the whole tool under one `timeout`.
Prints one JSON object.
"""
import argparse
import contextlib
import gc
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
sys.path.insert(0, SRC)
sys.path.insert(0, os.path.join(ROOT, "tools"))

A4 = (500000, 900000, 950000, 990000)
A8 = (250000, 500000, 750000, 900000, 950000, 990000, 995000, 999000)


def time_calls(H, W, calls=200, legs=5, warmup=20):
    import torch
    import stereo_device as sd
    rng = np.random.default_rng(H)
    gt = rng.uniform(0, 200, (H, W)).astype(np.float32)
    gt[rng.random((H, W)) < 0.1] = np.inf
    disp = (gt + rng.normal(0, 1.5, (H, W))).astype(np.float32)
    disp[~np.isfinite(disp)] = -1.0
    mask = rng.choice(np.array([0, 128, 255], np.uint8), size=(H, W), p=[0.05, 0.2, 0.75])
    d, g, m = (torch.from_numpy(a).cuda() for a in (disp, gt, mask))
    out, scratch = sd.evaluate_result("cuda"), sd.evaluate_scratch(H, W, "cuda")
    q_out, q_scratch = sd.evaluate_quantiles_result(d.device), sd.evaluate_quantiles_scratch(H, W, d.device)
    pool = sd.evaluate_quantiles_pool(d.device)
    variants = [
        ("evaluate", lambda: sd.evaluate(d, g, m, out=out, scratch=scratch)),
        ("quantiles_4", lambda: sd.evaluate_quantiles(d, g, m, A4, out=q_out, scratch=q_scratch)),
        ("quantiles_8", lambda: sd.evaluate_quantiles(d, g, m, A8, out=q_out, scratch=q_scratch)),
        ("pool_only", lambda: sd.evaluate_quantiles(d, g, m, A4, out=False, pool=pool, scratch=q_scratch)),
    ]
    for _, call in variants:
        for _ in range(warmup):
            call()
    us = {name: [] for name, _ in variants}
    for _ in range(legs):                                 # alternating legs
        for name, call in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                call()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / calls)
    median = {name: float(np.median(v)) for name, v in us.items()}
    return dict(height=H, width=W, bytes_read_per_pass=H * W * 9, calls_per_leg=calls,
                us_per_call={name: [round(x, 2) for x in v] for name, v in us.items()},
                median_us={name: round(v, 2) for name, v in median.items()},
                spread_us={name: round(max(v) - min(v), 2) for name, v in us.items()},
                ratio_to_evaluate={name: round(median[name] / median["evaluate"], 2) for name in median if name != "evaluate"})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--scenes", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[500, 750, 256], metavar=("H", "W", "NDISP"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--readers", type=int, default=4)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz"))
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    H, W, D = args.size
    import bench_evaluate
    import bench_list
    import match
    result = dict(tool="tools/bench_quantiles.py",
                  calls=[time_calls(500, 750, legs=args.legs), time_calls(1988, 2880, legs=args.legs)],
                  list=dict(pairs=args.pairs, height=H, width=W, ndisp=D, unit="ms per pair, wall, files written",
                            quantiles="50,90,95,99", passes={}))
    root = tempfile.mkdtemp(prefix="bench_quantiles_")
    try:
        lst = bench_list.write_list(root, args.pairs, args.scenes, H, W, D, 2000)
        bench_evaluate.add_truth(lst, 3000)
        variants = [("evaluate_a", []), ("evaluate_quantiles", ["--eval_quantiles", "50,90,95,99"]), ("evaluate_b", [])]

        def one_pass(name, extra):
            argv = ["-g", "0", "--list_file", lst, "--resume", args.weights, "--data_dir", os.path.join(root, "data"),
                    "--save_dir", os.path.join(root, "out_" + name), "-t", "b", "-s", "0", "-e", str(args.pairs - 1),
                    "--pipeline", "--readers", str(args.readers), "--evaluate"] + extra
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()):
                ret = match.main(argv)
            dt = time.time() - t0
            shutil.rmtree(os.path.join(root, "out_" + name), ignore_errors=True)
            del ret
            gc.collect()
            return dt * 1e3 / args.pairs

        for name, extra in variants:                      # untimed
            one_pass(name, extra)
        for _ in range(args.passes):                      # timed, alternating
            for name, extra in variants:
                result["list"]["passes"].setdefault(name, []).append(round(one_pass(name, extra), 3))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    summary = {}
    for name, ms in result["list"]["passes"].items():
        summary[name] = dict(mean=round(float(np.mean(ms)), 3), min=min(ms), max=max(ms), spread=round(max(ms) - min(ms), 3))
    result["list"]["summary"] = summary
    flagless = (summary["evaluate_a"]["mean"] + summary["evaluate_b"]["mean"]) / 2
    result["list"]["identical_legs_differ_by_ms_per_pair"] = round(abs(summary["evaluate_a"]["mean"]
                                                                       - summary["evaluate_b"]["mean"]), 3)
    result["list"]["quantiles_cost_ms_per_pair"] = round(summary["evaluate_quantiles"]["mean"] - flagless, 3)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
