#!/usr/bin/env python3
"""Aggregation with arms beyond 13 (cbca_distance 15 .. 32): the pixel-major kernel (mccnn_cbca_iter_hwd_long) against
the plane-major reference-order kernel it replaces on that range, per volume iteration and per whole pair.

One invocation measures ONE case (a scene and a distance) in ONE child process that runs under a time limit, and
merges the figures into profiles/long_arms.json:

    python tools/bench_long_arms.py --scene blobs+texture --L 28
    python tools/bench_long_arms.py --scene flat --L 28
    python tools/bench_long_arms.py --scene wide --L 28            # a 2880 x 200 x 256 window
    python tools/bench_long_arms.py --scene flat --L 28 --tree ../parent --label parent

Without --tree the case runs on this checkout: the time per volume iteration of both kernels (events around a chain
of one-volume launches), then the whole pair through StereoMatcher on the route the distance selects and through its
layout="plane_major" twin - the two alternate, leg by leg, in the one process, each leg after its own warm-up and at
least --seconds long - and the two final maps must be bit-identical.  With --tree the whole-pair figure of ANOTHER
checkout (built beforehand; its default StereoMatcher with the same hyper-parameters) is recorded under --label: the
yardstick for "no slower than before" is the parent commit, measured in the same session on the same device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"blobs+texture": (500, 750, 256, "blobs+texture"), "flat": (500, 750, 256, "flat"),
          "wide": (200, 2880, 256, "blobs+texture")}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", choices=sorted(SCENES), required=True)
    ap.add_argument("--L", type=int, required=True, help="cbca_distance")
    ap.add_argument("--seconds", type=float, default=2.0, help="least duration of a timed leg")
    ap.add_argument("--legs", type=int, default=2, help="legs per route (the routes alternate)")
    ap.add_argument("--tree", default=None, help="another built checkout to measure instead of this one")
    ap.add_argument("--label", default=None, help="key of the figures in the JSON file (default: this / the tree's name)")
    ap.add_argument("--timeout", type=int, default=240, help="time limit of the GPU step, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_arms.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def timed_leg(run, torch, seconds, warmup=3):
    """ms per call of `run` over at least `seconds` of back-to-back calls, after `warmup` calls."""
    for _ in range(warmup):
        out = run()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            out = run()
        n += 5
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3, n, out


def child(args):
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, os.path.join(tree, "mc-cnn-python_amd", "src"))
    import numpy as np
    import torch

    import _hipabi as hip
    import stereo_device as sd
    import synthetic
    import tf_checkpoint
    from model import NET

    hip.require_device()
    torch.cuda.set_device(0)
    H, W, D, kind = SCENES[args.scene]
    dist = args.L
    L, R = synthetic.make_pair(H, W, D, seed=100, kind=kind)[:2]
    l, r = torch.from_numpy(L[:, :, 0]).cuda(), torch.from_numpy(R[:, :, 0]).cuda()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(tree, "tests", "golden", "mccnn_fast_weights.npz")))
    hp = dict(cbca_distance=dist)
    res = {"shape_HWD": [H, W, D], "scene_kind": kind, "L": dist, "device": torch.cuda.get_device_properties(0).name}

    def matcher(**kw):
        m = sd.StereoMatcher(net, hp=hp, on_saturation="ignore", **kw)
        m.match_graph(l, r, D)             # eager warm-up, capture, first replay
        torch.cuda.synchronize()
        return m

    if args.tree:
        m = matcher()
        legs = [timed_leg(lambda: m.match_graph(l, r, D), torch, args.seconds)[0] for _ in range(args.legs)]
        res.update(pixel_major=bool(m.pixel_major()), ms_per_step_legs=[round(x, 3) for x in legs],
                   ms_per_step=round(min(legs), 3))
        print("RESULT " + json.dumps(res))
        return

    # ---- per volume iteration: events around a chain of one-volume launches --------------------------------------
    sup = sd.cross_arms(l, hp.get("cbca_intensity", 0.02), dist)
    arms = sup.view(torch.int32)[:H * W] if sup.dim() == 1 else sup.view(torch.int32)
    a4 = torch.stack([(arms >> s) & 31 for s in (0, 5, 10, 15)])
    res["share_of_pixels_with_an_arm_of_14_or_more"] = round(float((a4.max(0).values >= 14).float().mean()), 4)
    res["mean_region_pixels"] = round(float(((arms >> 20) & 0xfff).float().mean()), 1)
    g = torch.Generator(device="cuda").manual_seed(0)
    v = -torch.rand((D, H, W), device="cuda", generator=g) * 50
    hv = sd.dhw_to_hwd(v)
    t1, t2 = torch.empty_like(v), torch.empty_like(hv)

    def per_iteration(run, least=0.5):
        run(2)
        torch.cuda.synchronize()
        n, total = 4, 0.0
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(n)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= least * 1e3 or n >= 4096:
                return ms / n
            n *= 2

    ref = sd.cbca(v.clone(), t1, sup, 1, dist, hip.MCCNN_CBCA_REFERENCE_ORDER)[0]
    got = sd.cbca_hwd(hv.clone(), t2, sup, D, 1, dist)[0]
    assert torch.equal(sd.hwd_to_dhw(got, D), ref), "the two kernels disagree on one iteration"
    del ref, got
    res["ms_per_volume_iteration_hwd_long"] = round(per_iteration(lambda n: sd.cbca_hwd(hv, t2, sup, D, n, dist)), 4)
    res["ms_per_volume_iteration_plane_major"] = round(
        per_iteration(lambda n: sd.cbca(v, t1, sup, n, dist, hip.MCCNN_CBCA_REFERENCE_ORDER)), 4)
    del v, hv, t1, t2
    torch.cuda.empty_cache()

    # ---- whole pair: the two routes alternate ----------------------------------------------------------------------
    new, old = matcher(), matcher(layout="plane_major")
    res["route"] = new.route(H, W, D)
    assert new.pixel_major() and not old.pixel_major()
    legs = {"new": [], "plane_major": []}
    maps = {}
    for _ in range(args.legs):
        for name, m in (("new", new), ("plane_major", old)):
            ms, _n, out = timed_leg(lambda: m.match_graph(l, r, D), torch, args.seconds)
            legs[name].append(round(ms, 3))
            maps[name] = out.clone()
    a, b = maps["new"].cpu().numpy(), maps["plane_major"].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the final maps of the two routes differ"
    res.update(ms_per_step_legs=legs["new"], ms_per_step=min(legs["new"]),
               ms_per_step_plane_major_legs=legs["plane_major"], ms_per_step_plane_major=min(legs["plane_major"]),
               final_maps_bit_identical=True)
    print("RESULT " + json.dumps(res))


def main():
    args = parse()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = p.stdout.decode()
    line = next((ln for ln in text.splitlines() if ln.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        sys.stderr.write(text[-4000:])
        raise SystemExit("bench_long_arms: the GPU step ended with status %d" % p.returncode)
    res = json.loads(line[len("RESULT "):])
    label = args.label or ("this" if not args.tree else os.path.basename(os.path.abspath(args.tree)))
    data = {}
    if os.path.isfile(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data.setdefault("%s/L=%d" % (args.scene, args.L), {})[label] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"case": "%s/L=%d" % (args.scene, args.L), "label": label, **res}))


if __name__ == "__main__":
    main()
