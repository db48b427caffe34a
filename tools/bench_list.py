#!/usr/bin/env python3
"""Times match.py over a LIST of pairs: the flagless list loop against --pipeline (each also with --pairs_in_flight 2).

    timeout -k 10 900 python tools/bench_list.py [--pairs 100] [--scenes 10] [--size 500 750 256] [--readers 4]
                                                 [--baseline-src DIR | --compare-src DIR] [--out FILE]

Writes a seeded list of synthetic PNG pairs (synthetic.make_scene_u8; `--scenes` different scenes, written over and over
until there are `--pairs` entries - nothing in either loop caches a pair) into a temporary directory and runs the list,
in ONE process, through match.main(argv): one untimed pass of each variant, then three timed passes of each,
alternating, a host clock around each call (main returns only when every file is written).  Graph capture is inside the
timed passes: a user pays it.  Any exception ends the tool there - nothing further is started on the GPU; run the whole
tool under one `timeout`.  Prints one JSON object.

--baseline-src DIR: the flagless variants run the match.py of another source tree (e.g. the parent commit's
mc-cnn-python_amd/src, exported with `git archive`) against the same built library, so that the baseline is not a
variant of the code under test.

--compare-src DIR: another question - has the host code of the loops become slower?  Every loop (flagless, flagless with
--pairs_in_flight 2, --pipeline) runs as three legs, alternating: DIR, DIR again, this tree.  The two identical legs are
the yardstick: a loop passes when this tree's mean differs from the mean of DIR's two legs by no more than those two
legs' means differ from each other.  Exit status 0 when every loop passes.
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


@contextlib.contextmanager
def source_tree(src, stash):
    """Imports inside the block resolve the package's module names (match, stereo_device, ...) in `src`; `stash` keeps
    that tree's modules between blocks.  Other modules (torch, numpy) are shared."""
    names = {os.path.splitext(f)[0] for d in (SRC, src) for f in os.listdir(d) if f.endswith(".py")}
    outside = {n: sys.modules.pop(n) for n in names if n in sys.modules}
    sys.modules.update(stash)
    sys.path.insert(0, src)
    try:
        yield
    finally:
        sys.path.remove(src)
        stash.clear()
        stash.update({n: sys.modules.pop(n) for n in names if n in sys.modules})
        sys.modules.update(outside)


def write_list(root, pairs, scenes, H, W, D, seed, truth=False):
    from PIL import Image
    sys.path.insert(0, SRC)
    import synthetic
    import util
    sys.path.remove(SRC)
    made = []
    for s in range(scenes):
        left, right, disparity = synthetic.make_scene_u8(H, W, D, seed=seed + s)
        made.append((left, right, np.asarray(disparity, np.float32)))
    lines = []
    for i in range(pairs):
        d = os.path.join(root, "data", "set", "pair%03d" % i)
        os.makedirs(d)
        left, right, disparity = made[i % scenes]
        Image.fromarray(left, mode="L").save(os.path.join(d, "im0.png"))
        Image.fromarray(right, mode="L").save(os.path.join(d, "im1.png"))
        if truth:        # (what the figures say is not the point: the scoring path is inside the timing)
            util.writePfm(disparity, os.path.join(d, "disp0GT.pfm"))
            util.writePfm(disparity, os.path.join(d, "disp1GT.pfm"))
        with open(os.path.join(d, "calib.txt"), "w") as f:
            f.write("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                    "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (W, H, D, D))
        lines.append(os.path.join(d, "im0.png"))
    lst = os.path.join(root, "list.txt")
    with open(lst, "w") as f:
        f.write("".join(p + "\n" for p in lines))
    return lst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=3, default=[500, 750, 256], metavar=("H", "W", "NDISP"))
    ap.add_argument("--readers", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--baseline-src", default=None, help="source tree whose match.py runs the flagless variants")
    ap.add_argument("--compare-src", default=None,
                    help="source tree (the parent commit's) that every loop is compared with; see above")
    ap.add_argument("--truth", action="store_true", help="the list carries disp0GT.pfm and disp1GT.pfm beside every pair")
    ap.add_argument("--flags", default="", help="more match.py flags for every variant, e.g. '--evaluate --views both'")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz"))
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    H, W, D = args.size
    if args.baseline_src or args.compare_src:
        # the other tree's binding looks for the library beside itself: point both at the one that was built here
        os.environ.setdefault("MCCNN_HIP_LIB", os.path.join(ROOT, "mc-cnn-python_amd", "lib", "libmccnn_hip.so"))
    base_src = os.path.abspath(args.baseline_src) if args.baseline_src else SRC
    stashes = {SRC: {}, base_src: {}}
    variants = [("flagless", base_src, []), ("flagless_in_flight_2", base_src, ["--pairs_in_flight", "2"]),
                ("pipeline", SRC, ["--pipeline", "--readers", str(args.readers)]),
                ("pipeline_in_flight_2", SRC, ["--pipeline", "--readers", str(args.readers), "--pairs_in_flight", "2"])]
    if args.compare_src:
        other = os.path.abspath(args.compare_src)
        stashes[other] = {}
        variants = [("%s@%s" % (name, leg), src, extra) for name, _, extra in variants[:3]
                    for leg, src in (("parent_a", other), ("parent_b", other), ("branch", SRC))]
    root = tempfile.mkdtemp(prefix="bench_list_")
    result = dict(tool="tools/bench_list.py", pairs=args.pairs, scenes=args.scenes, height=H, width=W, ndisp=D,
                  readers=args.readers, truth=args.truth, flags=args.flags, baseline_src="parent export" if args.baseline_src else "this tree",
                  unit="ms per pair, wall, files written", passes={}, counters={}, stage_seconds_last_pass={}, steady_ms_per_pair_last_pass={})
    try:
        t = time.time()
        lst = write_list(root, args.pairs, args.scenes, H, W, D, args.seed, args.truth)
        result["list_written_s"] = round(time.time() - t, 2)

        def one_pass(name, src, extra, tag):
            argv = ["-g", "0", "--list_file", lst, "--resume", args.weights, "--data_dir", os.path.join(root, "data"),
                    "--save_dir", os.path.join(root, "out_" + name), "-t", tag, "-s", "0", "-e", str(args.pairs - 1)] + extra + args.flags.split()
            with source_tree(src, stashes[src]):
                import match
                log = io.StringIO()
                t0 = time.time()
                with contextlib.redirect_stdout(log):
                    ret = match.main(argv)
                dt = time.time() - t0
            shutil.rmtree(os.path.join(root, "out_" + name), ignore_errors=True)
            if ret is not None and hasattr(ret, "counters"):
                result["counters"][name] = dict(ret.counters)
                result["stage_seconds_last_pass"][name] = {k: round(v, 3) for k, v in ret.seconds.items()}
                result["stage_seconds_last_pass"][name]["whole_pass"] = round(dt, 3)
                at = ret.submitted_at
                if len(at) > 20:     # submit to submit behind the first ten pairs (eager pair, warm-ups, capture)
                    result["steady_ms_per_pair_last_pass"][name] = round((at[-1] - at[10]) * 1e3 / (len(at) - 11), 3)
            del ret
            gc.collect()                                       # the pass's matchers, workspaces and graphs go now
            return dt * 1e3 / args.pairs

        for name, src, extra in variants:                      # untimed
            one_pass(name, src, extra, "warm")
        for k in range(args.passes):                           # timed, alternating
            for name, src, extra in variants:
                result["passes"].setdefault(name, []).append(round(one_pass(name, src, extra, "t%d" % k), 3))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    summary = {}
    for name, ms in result["passes"].items():
        summary[name] = dict(mean=round(float(np.mean(ms)), 3), min=min(ms), max=max(ms), spread=round(max(ms) - min(ms), 3))
    result["summary"] = summary
    if args.compare_src:
        result["baseline_src"] = "parent export, every loop (--compare-src)"
        result["compare"] = {}
        for loop in sorted({name.split("@")[0] for name in summary}):
            a, b, mine = (summary["%s@%s" % (loop, leg)]["mean"] for leg in ("parent_a", "parent_b", "branch"))
            result["compare"][loop] = dict(parent=round((a + b) / 2, 3), branch=mine, difference=round(mine - (a + b) / 2, 3),
                                           yardstick=round(abs(a - b), 3), within=bool(abs(mine - (a + b) / 2) <= abs(a - b)))
        result["every_loop_within_the_yardstick"] = all(c["within"] for c in result["compare"].values())
        return finish(args, result, result["every_loop_within_the_yardstick"])
    base, pipe = summary["flagless"], summary["pipeline"]
    result["pipeline_gain_ms_per_pair"] = round(base["mean"] - pipe["mean"], 3)
    result["baseline_spread_ms"] = base["spread"]
    result["pipeline_faster_by_more_than_baseline_spread"] = bool(base["mean"] - pipe["mean"] > base["spread"])
    return finish(args, result, result["pipeline_faster_by_more_than_baseline_spread"])


def finish(args, result, passed):
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if passed else 1


if __name__ == "__main__":
    sys.exit(main())
