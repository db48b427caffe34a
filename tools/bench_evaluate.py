#!/usr/bin/env python3
"""Times the device-side evaluation (csrc/evaluate.hip) and what match.py --evaluate costs a streamed list.

    timeout -k 10 900 python tools/bench_evaluate.py [--pairs 40] [--size 500 750 256] [--out profiles/evaluate.json]

1. stereo_device.evaluate on a 750 x 500 and a 2880 x 1988 map (mask, four thresholds): HIP events around batches of 200
   calls behind 20 warm-up calls, five batches, median and spread - microseconds per call, both launches.
2. A seeded list of synthetic pairs with a ground truth and a mask beside each (tools/bench_list.py's writer), run in ONE
   process through match.main(argv) with --pipeline, with and without --evaluate: one untimed pass of each, then
   `--passes` timed passes of each, alternating, a host clock around each call - ms per pair, files written.
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


def time_kernel(H, W, calls=200, batches=5, warmup=20):
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
    for _ in range(warmup):
        sd.evaluate(d, g, m, out=out, scratch=scratch)
    us = []
    for _ in range(batches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            sd.evaluate(d, g, m, out=out, scratch=scratch)
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / calls)
    return dict(height=H, width=W, bytes_read=H * W * 9, calls_per_batch=calls, us_per_call=[round(x, 2) for x in us],
                median_us=round(float(np.median(us)), 2), spread_us=round(max(us) - min(us), 2))


def add_truth(lst, seed):
    from PIL import Image
    import util
    rng = np.random.default_rng(seed)
    for left in open(lst).read().split():
        d = os.path.dirname(left)
        W, H = Image.open(left).size
        gt = rng.uniform(0, 200, (H, W)).astype(np.float32)
        gt[rng.random((H, W)) < 0.1] = np.inf
        util.writePfm(gt, os.path.join(d, "disp0GT.pfm"))
        mask = rng.choice(np.array([0, 128, 255], np.uint8), size=(H, W), p=[0.05, 0.2, 0.75])
        Image.fromarray(mask, mode="L").save(os.path.join(d, "mask0nocc.png"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--scenes", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[500, 750, 256], metavar=("H", "W", "NDISP"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--readers", type=int, default=4)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz"))
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    H, W, D = args.size
    import bench_list
    import match
    result = dict(tool="tools/bench_evaluate.py", kernel=[time_kernel(500, 750), time_kernel(1988, 2880)],
                  list=dict(pairs=args.pairs, height=H, width=W, ndisp=D, unit="ms per pair, wall, files written",
                            passes={}))
    root = tempfile.mkdtemp(prefix="bench_evaluate_")
    try:
        lst = bench_list.write_list(root, args.pairs, args.scenes, H, W, D, 2000)
        add_truth(lst, 3000)
        variants = [("pipeline", []), ("pipeline_evaluate", ["--evaluate"])]

        def one_pass(name, extra):
            argv = ["-g", "0", "--list_file", lst, "--resume", args.weights, "--data_dir", os.path.join(root, "data"),
                    "--save_dir", os.path.join(root, "out_" + name), "-t", "b", "-s", "0", "-e", str(args.pairs - 1),
                    "--pipeline", "--readers", str(args.readers)] + extra
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
    result["list"]["evaluate_cost_ms_per_pair"] = round(summary["pipeline_evaluate"]["mean"] - summary["pipeline"]["mean"], 3)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
