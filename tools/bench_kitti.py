#!/usr/bin/env python3
"""Times the KITTI path: the kernels of csrc/kitti.hip alone, and match.py --pipeline over a list from a KITTI tree
against the same images as a Middlebury tree.

    timeout -k 10 600 python tools/bench_kitti.py [--pairs 20] [--scenes 4] [--size 375 1242 228] [--out profiles/kitti.json]

The parent process never touches the GPU.  It writes the two synthetic trees (synthetic.make_scene_u8, colour PNGs, the
same files in both) and then runs two steps, each a fresh child process under a time limit of its own:
    kernels     encode, decode, background interpolation (a map with 10 % holes in runs) and the scorer with and without
                interpolation at H x W: device time per call from events around 200 back-to-back calls behind 20 untimed ones
    lists       in ONE process, match.main(--pipeline --dataset kitti2015 --ndisp D) over the KITTI list and
                match.main(--pipeline) over the Middlebury list: one untimed pass of each, then --passes timed passes of
                each, alternating, a host clock around each call (main returns only when every file is written)
A step that fails or runs out of time ends the tool there: nothing further is started on the GPU.  The figure to watch is
the KITTI list's time per pair against the Middlebury list's, and in the stage seconds of the last pass `writer_files`:
the 16-bit PNG is compressed on the writer thread where the PFM is a plain write.  Prints one JSON object.
"""
import argparse
import contextlib
import gc
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
CALIB = ("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
         "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")
STEP_LIMITS = dict(kernels=120, lists=400)      # seconds


def write_trees(root, pairs, scenes, H, W, D, seed):
    from PIL import Image
    sys.path.insert(0, SRC)
    import synthetic
    made = [synthetic.make_scene_u8(H, W, D, seed=seed + s)[:2] for s in range(scenes)]
    k15, mb = os.path.join(root, "kitti", "training"), os.path.join(root, "middlebury", "set")
    for d in ("image_2", "image_3"):
        os.makedirs(os.path.join(k15, d))
    lists = {"kitti": [], "middlebury": []}
    for i in range(pairs):
        pair = os.path.join(mb, "pair%03d" % i)
        os.makedirs(pair)
        name = "%06d_10.png" % i
        for view, mb_name, img in zip(("image_2", "image_3"), ("im0.png", "im1.png"), made[i % scenes]):
            Image.fromarray(np.repeat(img[:, :, None], 3, axis=2), mode="RGB").save(os.path.join(k15, view, name))
            shutil.copyfile(os.path.join(k15, view, name), os.path.join(pair, mb_name))
        with open(os.path.join(pair, "calib.txt"), "w") as f:
            f.write(CALIB % (W, H, D, D))
        lists["kitti"].append(os.path.join(k15, "image_2", name))
        lists["middlebury"].append(os.path.join(pair, "im0.png"))
    for which, lines in lists.items():
        with open(os.path.join(root, which + ".txt"), "w") as f:
            f.write("".join(p + "\n" for p in lines))


def step_kernels(args):
    sys.path.insert(0, SRC)
    import torch
    import stereo_device as sd
    sd.hip.require_device()
    H, W, _ = args.size
    rng = np.random.default_rng(args.seed)
    disp = rng.uniform(0, 200, (H, W)).astype(np.float32)
    for _ in range(H * W // 100):                         # 10 % holes, in runs of ten
        v, u = int(rng.integers(0, H)), int(rng.integers(0, W))
        disp[v, u:u + 10] = -1.0
    occ = (rng.integers(1, 200 * 256, (H, W)) * (rng.random((H, W)) < 0.3)).astype(np.uint16)
    d, o = torch.from_numpy(disp).cuda(), torch.from_numpy(occ).cuda()
    code, back, filled, result = sd.kitti_encode_u16(d), torch.empty_like(d), torch.empty_like(d), sd.evaluate_result(d.device)
    scratch = sd.evaluate_kitti_scratch(H, W, d.device, True)
    calls = dict(encode_u16=lambda: sd.kitti_encode_u16(d, out=code),
                 decode_u16=lambda: sd.kitti_decode_u16(code, out=back),
                 interpolate_background=lambda: sd.kitti_interpolate_background(d, out=filled),
                 evaluate_kitti=lambda: sd.evaluate_kitti(d, o, o, out=result, scratch=scratch),
                 evaluate_kitti_interpolate=lambda: sd.evaluate_kitti(d, o, o, interpolate=True, out=result, scratch=scratch))
    out = {}
    for name, call in calls.items():
        for _ in range(20):
            call()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(200):
            call()
        end.record()
        end.synchronize()
        out[name] = round(start.elapsed_time(end) * 1e3 / 200, 2)
    return dict(unit="us per call, 200 back-to-back calls (launch overhead of the host loop included)", height=H, width=W,
                device=torch.cuda.get_device_name(0), **out)


def step_lists(args):
    sys.path.insert(0, SRC)
    import match
    H, W, D = args.size
    out = {which: dict(passes_ms_per_pair=[]) for which in ("kitti", "middlebury")}
    for k in range(args.passes + 1):                        # the first pass of each is untimed
        for which in ("kitti", "middlebury"):
            extra = ["--dataset", "kitti2015", "--ndisp", str(D)] if which == "kitti" else []
            save = os.path.join(args.root, "out_" + which)
            argv = ["-g", "0", "--list_file", os.path.join(args.root, which + ".txt"), "--resume", args.weights,
                    "--data_dir", os.path.join(args.root, which), "--save_dir", save, "-t", "p%d" % k, "-s", "0", "-e",
                    str(args.pairs - 1), "--pipeline", "--readers", str(args.readers)] + extra
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()):
                pipeline = match.main(argv)
            dt = time.time() - t0
            nbytes = sum(os.path.getsize(os.path.join(d, f)) for d, _dirs, files in os.walk(os.path.join(save, "submit_p%d" % k))
                         for f in files if f.endswith((".png", ".pfm")))
            shutil.rmtree(save, ignore_errors=True)
            if k > 0:
                o = out[which]
                o["passes_ms_per_pair"].append(round(dt * 1e3 / args.pairs, 3))
                o["counters"] = dict(pipeline.counters)
                o["stage_seconds_last_pass"] = {name: round(v, 3) for name, v in pipeline.seconds.items()}
                o["map_file_bytes_per_pair"] = nbytes // args.pairs
            del pipeline
            gc.collect()                                    # the pass's matchers, workspaces and graphs go now
    for o in out.values():
        o["mean_ms_per_pair"] = round(float(np.mean(o["passes_ms_per_pair"])), 3)
        o["writer_files_ms_per_pair"] = round(o["stage_seconds_last_pass"]["writer_files"] * 1e3 / args.pairs, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=3, default=[375, 1242, 228], metavar=("H", "W", "NDISP"))
    ap.add_argument("--readers", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2000)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti.json"))
    ap.add_argument("--step", choices=tuple(STEP_LIMITS), default=None, help=argparse.SUPPRESS)   # a child of this tool
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        result = step_kernels(args) if args.step == "kernels" else step_lists(args)
        print("RESULT " + json.dumps(result))
        return 0
    H, W, D = args.size
    root = tempfile.mkdtemp(prefix="bench_kitti_")
    result = dict(tool="tools/bench_kitti.py", pairs=args.pairs, scenes=args.scenes, height=H, width=W, ndisp=D,
                  readers=args.readers, passes=args.passes, unit="ms per pair, wall, files written")
    status = 0
    try:
        t = time.time()
        write_trees(root, args.pairs, args.scenes, H, W, D, args.seed)
        result["trees_written_s"] = round(time.time() - t, 2)
        passed = [a for a in sys.argv[1:]]
        for step, limit in STEP_LIMITS.items():
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--step", step, "--root", root]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
            except subprocess.TimeoutExpired:
                result[step] = dict(failed="no result within %d s" % limit)
                status = 1
                break
            lines = [line for line in r.stdout.decode().splitlines() if line.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                result[step] = dict(failed="exit status %d" % r.returncode, tail=r.stdout.decode()[-1500:])
                status = 1
                break                                       # nothing further is started on the GPU
            result[step] = json.loads(lines[-1][len("RESULT "):])
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if status == 0:
        k, m = result["lists"]["kitti"], result["lists"]["middlebury"]
        result["kitti_minus_middlebury_ms_per_pair"] = round(k["mean_ms_per_pair"] - m["mean_ms_per_pair"], 3)
        result["middlebury_spread_ms"] = round(max(m["passes_ms_per_pair"]) - min(m["passes_ms_per_pair"]), 3)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return status


if __name__ == "__main__":
    sys.exit(main())
