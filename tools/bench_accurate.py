"""The accurate network on one synthetic pair (default 750x500, 256 disparities; Middlebury-accurate topology: 5 conv
layers of 112 maps, 3 fully-connected layers of 384 units; seeded glorot weights): per-pair time of the three decision
routes - float32 library matmuls, the split-operand kernel, the plain-f16 kernel - measured alternately in ONE process
after a warm-up, the decision stage alone (TFLOP/s) and per-stage times, plus the f16 precision's end-to-end effect
against the default precision.  Prints one JSON object (kept as profiles/accurate.json).

    python tools/bench_accurate.py [--height 500 --width 750 --ndisp 256 --passes 3] [--out FILE]
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
from model import ACCURATE_NET

F16_DENSE_PEAK_TFLOPS = 2500.0      # MI355X f16 matrix peak (dense), for the "fraction of peak" figures


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=[round(x, 3) for x in xs])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=750)
    ap.add_argument("--ndisp", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3, help="timed passes of each route (at least 3)")
    ap.add_argument("--num_fc_layers", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON object to this file")
    args = ap.parse_args(argv)
    passes = max(3, args.passes)
    hip.require_device()
    torch.cuda.set_device(0)
    H, W, D = args.height, args.width, args.ndisp
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=3)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    net = ACCURATE_NET(None, batch_size=1, device="cuda", seed=0, num_fc_layers=args.num_fc_layers)
    routes = {
        "library_f32": dict(decision="library", cv_mode=hip.MCCNN_CV_EXACT),
        "kernel_split": dict(decision="kernel", cv_mode=hip.MCCNN_CV_EXACT),
        "kernel_f16": dict(decision="kernel", cv_mode=hip.MCCNN_CV_MFMA),
    }
    matchers = {k: sd.StereoMatcher(net, on_saturation="ignore", **kw) for k, kw in routes.items()}

    # the decision stage alone, on the tower outputs of the pair
    fl, fr = net.features_pair_hwc(dl[:, :, 0].contiguous(), dr[:, :, 0].contiguous())
    dp = sd.hwd_pitch(D)
    vols = tuple(torch.empty((H, W, dp), dtype=torch.float32, device="cuda") for _ in range(2))
    halves = tuple(torch.empty((H, W, net.num_fc_units), dtype=torch.float32, device="cuda") for _ in range(2))
    voxels = sum(H * (W - d) for d in range(D))
    u, nl = net.num_fc_units, net.num_fc_layers - 1
    flop = 2.0 * voxels * (nl * u * u + u)            # layers 2 .. n_fc and the final product, plain multiply-adds
    stage = {k: [] for k in routes}

    def run_stage(k):
        kw = routes[k]
        return sd.cost_volume_accurate(net, fl, fr, D, mode=kw["cv_mode"], decision=kw["decision"], pixel_major=True,
                                       out=vols, halves=halves)

    pair = {k: [] for k in routes}
    for k in routes:                                   # warm-up: library kernels chosen, weights packed, workspaces
        run_stage(k)
        matchers[k].match(dl, dr, D)
    torch.cuda.synchronize()
    for _ in range(passes):                            # alternately, so that drift hits every route alike
        for k in routes:
            stage[k].append(timed(lambda: run_stage(k))[0])
        for k in routes:
            pair[k].append(timed(lambda: matchers[k].match(dl, dr, D))[0])

    result = dict(shape=dict(height=H, width=W, ndisp=D), topology=dict(conv_layers=net.num_conv_layers,
                  feature_maps=net.num_conv_feature_maps, fc_layers=net.num_fc_layers, fc_units=u),
                  voxels=voxels, decision_flop=flop, passes=passes, per_pair_ms={}, decision_stage_ms={},
                  decision_stage_tflops={}, fraction_of_f16_peak={})
    for k in routes:
        result["per_pair_ms"][k] = spread(pair[k])
        result["decision_stage_ms"][k] = spread(stage[k])
        med = statistics.median(stage[k])
        mult = 3.0 if k == "kernel_split" else 1.0     # three f16 products per multiply
        result["decision_stage_tflops"][k] = flop / (med * 1e-3) / 1e12
        if k != "library_f32":
            result["fraction_of_f16_peak"][k] = mult * flop / (med * 1e-3) / 1e12 / F16_DENSE_PEAK_TFLOPS
    result["kernel_not_slower_than_library"] = bool(
        result["per_pair_ms"]["kernel_split"]["median"] <= result["per_pair_ms"]["library_f32"]["median"])
    result["decision_auto"] = sd.DECISION_AUTO

    # per-stage times of one pair on the default route (nothing overlaps under the timer)
    timer = sd.StageTimer(True)
    matchers["kernel_split"].match(dl, dr, D, timer=timer)
    torch.cuda.synchronize()
    result["stages_ms"] = {k: round(sum(v), 3) for k, v in timer.summary_ms().items()}
    result["stage_spans_ms"] = {k: round(sum(v), 3) for k, v in timer.spans_ms().items()}

    # the f16 precision end to end against the default precision (recorded, not gated)
    keeps = {}
    for k in ("kernel_split", "kernel_f16"):
        keeps[k] = {}
        matchers[k].match(dl, dr, D, keep=keeps[k])
    torch.cuda.synchronize()
    a, b = keeps["kernel_split"], keeps["kernel_f16"]
    diff = (a["bilateral"] - b["bilateral"]).abs().flatten().double()
    cvd = (a["cv"][0] - b["cv"][0]).abs().max()
    result["f16_vs_default"] = dict(
        wta_flips_left=int((a["wta"][0] != b["wta"][0]).sum()), wta_flips_right=int((a["wta"][1] != b["wta"][1]).sum()),
        pixels=H * W, frac_within_1e3_px=float((diff <= 1e-3).double().mean()),
        p99_abs_px=float(torch.quantile(diff, 0.99)), cost_volume_max_abs=float(cvd))
    text = json.dumps(result, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return result


if __name__ == "__main__":
    main()
