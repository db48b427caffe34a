"""The paper-faithful SGM stage (four independent directions accumulated out of place, mccnn_sgm_pass_accumulate) beside
the reference's sequential stage (four passes in place, mccnn_sgm_pass_flagged), measured alternately in ONE process
after a warm-up, with device events.  For the main shape (default 750x500, 256 disparities):

  passes      every direction's kernel time in both forms, one-volume and two-volume launches, and the bytes/s each
              achieves: by the algorithm an in-place pass moves 8 B/voxel (read + write), the storing pass 8 (source read,
              accumulator written), an adding pass 12 (source and accumulator read, accumulator written)
  stage       the four passes of both volumes back to back (44 B/voxel against 32); the target is
              stage_independent <= 44/32 x stage_in_place x 1.15 of the same run
  chain span  the SGM bracket of one free-running chain inside a whole pair (StageTimer spans)
  pair        whole-pair time with and without the extra sgm_independent_directions

and passes + stage for the other shapes (default 1242x375x192 and 1500x1000x400: three disparities per lane, two groups
per lane).  Prints one JSON object (kept as profiles/paper_sgm.json).

    python tools/bench_paper_sgm.py [--height 500 --width 750 --ndisp 256 --passes 7] [--also 1242x375x192,1500x1000x400]
                                    [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

import torch

import _hipabi as hip
import stereo_device as sd
import synthetic
import tf_checkpoint
from model import NET

SGM_HP = (2.3, 55.9, 4, 8, 0.08, 1.5)
NAMES = ("right", "left", "up", "bottom")
ACC_BYTES = {hip.MCCNN_SGM_ACC_STORE: 8, hip.MCCNN_SGM_ACC_ADD: 12, hip.MCCNN_SGM_ACC_ADD_QUARTER: 12}
TARGET = 44.0 / 32.0 * 1.15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4),
                runs=[round(x, 4) for x in xs])


def sgm_stage(H, W, D, passes):
    """Kernel times of the passes and of the whole stage, both forms, on random volumes of the shape."""
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(D)
    dp = sd.hwd_pitch(D)
    l = torch.randn((H, W), device=dev, generator=g) * 0.07
    r = torch.randn((H, W), device=dev, generator=g) * 0.07
    src = [torch.rand((H, W, dp), device=dev, generator=g) for _ in range(2)]
    work = [s.clone() for s in src]                      # what the in-place passes chew on
    acc = [torch.empty_like(s) for s in src]
    planes = sd.sgm_flag_planes(l, r, D, SGM_HP[4])
    p1h, p1v, p2, q1, q2, _thr = sd._sgm_penalties(*SGM_HP)
    sides = [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT]
    voxels = H * W * dp

    def in_place(i, n):
        rr = sd.SGM_DIRECTIONS[i]
        sd.sgm_pass_flagged_hwd(work[:n], sides[:n], D, rr, p1h if rr[0] == 0 else p1v, p2, q1, q2, planes[i])

    def accumulate(i, n):
        rr = sd.SGM_DIRECTIONS[i]
        sd.sgm_pass_accumulate_hwd(src[:n], acc[:n], sides[:n], D, rr, p1h if rr[0] == 0 else p1v, p2, q1, q2,
                                   sd.SGM_ACC_MODES[i], planes[i])

    def restore():                                       # the in-place passes grow their volume without bound otherwise
        for w, s in zip(work, src):
            w.copy_(s)

    runs = {}
    for warm in (True, False):                           # one untimed round, then the timed ones, alternating the forms
        for _ in range(1 if warm else passes):
            restore()
            for n in (1, 2):
                for i, name in enumerate(NAMES):
                    for form, fn in (("in_place", in_place), ("accumulate", accumulate)):
                        ms = timed(lambda: fn(i, n))[0]
                        if not warm:
                            runs.setdefault((form, name, n), []).append(ms)
            restore()
            for form, fn in (("in_place", in_place), ("accumulate", accumulate)):
                ms = timed(lambda: [fn(i, 2) for i in range(4)])[0]
                if not warm:
                    runs.setdefault((form, "stage", 2), []).append(ms)
    out = dict(shape=dict(height=H, width=W, ndisp=D), voxels_per_volume=voxels, passes={}, stage_ms={})
    for i, name in enumerate(NAMES):
        for n in (1, 2):
            a, b = runs[("in_place", name, n)], runs[("accumulate", name, n)]
            ma, mb = statistics.median(a), statistics.median(b)
            bytes_a, bytes_b = 8.0 * voxels * n, float(ACC_BYTES[sd.SGM_ACC_MODES[i]]) * voxels * n
            out["passes"]["%s_%dvol" % (name, n)] = dict(
                in_place_ms=spread(a), accumulate_ms=spread(b), accumulate_mode=int(sd.SGM_ACC_MODES[i]),
                in_place_gb_per_s=round(bytes_a / (ma * 1e-3) / 1e9, 1), accumulate_gb_per_s=round(bytes_b / (mb * 1e-3) / 1e9, 1),
                accumulate_bandwidth_over_in_place=round((bytes_b / mb) / (bytes_a / ma), 3))
    a, b = runs[("in_place", "stage", 2)], runs[("accumulate", "stage", 2)]
    ratio = statistics.median(b) / statistics.median(a)
    out["stage_ms"] = dict(in_place=spread(a), independent=spread(b), ratio=round(ratio, 3), target_ratio=round(TARGET, 3),
                           within_target=bool(ratio <= TARGET),
                           in_place_gb_per_s=round(32.0 * voxels * 2 / (statistics.median(a) * 1e-3) / 1e9, 1),
                           independent_gb_per_s=round(44.0 * voxels * 2 / (statistics.median(b) * 1e-3) / 1e9, 1))
    return out


def whole_pair(H, W, D, passes):
    """Whole-pair time and the per-chain SGM span with and without the extra."""
    layers = tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz"))
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(layers)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=3)
    dl, dr = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
    matchers = {"sequential": sd.StereoMatcher(net, on_saturation="ignore"),
                "independent": sd.StereoMatcher(net, on_saturation="ignore", extras=dict(sgm_independent_directions=True))}
    outs = {k: torch.empty((H, W), dtype=torch.float32, device="cuda") for k in matchers}
    for k, m in matchers.items():
        for _ in range(2):
            m.match(dl, dr, D, out=outs[k])
    torch.cuda.synchronize()
    pair = {k: [] for k in matchers}
    spans = {k: [] for k in matchers}
    for _ in range(passes):
        for k, m in matchers.items():
            pair[k].append(timed(lambda: m.match(dl, dr, D, out=outs[k]))[0])
    for _ in range(passes):
        for k, m in matchers.items():
            timer = sd.StageTimer(True)
            m.match(dl, dr, D, timer=timer, out=outs[k])
            torch.cuda.synchronize()
            spans[k].extend(timer.spans_ms().get("sgm", []))
    return dict(shape=dict(height=H, width=W, ndisp=D),
                pair_ms={k: spread(v) for k, v in pair.items()},
                sgm_chain_span_ms={k: spread(v) for k, v in spans.items()},
                pair_ms_added_by_the_extra=round(statistics.median(pair["independent"]) - statistics.median(pair["sequential"]), 4),
                maps_differ=bool((outs["sequential"] != outs["independent"]).any()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=750)
    ap.add_argument("--ndisp", type=int, default=256)
    ap.add_argument("--passes", type=int, default=7, help="timed rounds of each variant (at least 3)")
    ap.add_argument("--also", type=str, default="1242x375x192,1500x1000x400",
                    help="WxHxD[,WxHxD...]: passes and stage for these shapes too ('' for none)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON object to this file")
    args = ap.parse_args(argv)
    passes = max(3, args.passes)
    hip.require_device()
    torch.cuda.set_device(0)
    H, W, D = args.height, args.width, args.ndisp
    result = dict(passes_per_variant=passes, device=torch.cuda.get_device_name(0),
                  library=os.path.relpath(hip.LIB_PATH, ROOT), main=sgm_stage(H, W, D, passes), other_shapes=[])
    result["main"]["whole_pair"] = whole_pair(H, W, D, passes)
    for spec in [s for s in args.also.split(",") if s]:
        w, h, d = (int(x) for x in spec.split("x"))
        result["other_shapes"].append(sgm_stage(h, w, d, passes))
        torch.cuda.empty_cache()
    print(json.dumps(result, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    return result


if __name__ == "__main__":
    main()
