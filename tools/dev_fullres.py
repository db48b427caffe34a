#!/usr/bin/env python3
"""Dev harness (GPU box): a synthetic pair of full-resolution Middlebury shape through StereoMatcher.match, with
per-stage times, and every SGM direction timed alone on one volume (against 8 TB/s on the algorithmic 8 bytes per
voxel and pass: one read and one write of the volume).

    python tools/dev_fullres.py                         # 2880x1988x800 and 2880x1988x256
    python tools/dev_fullres.py 3072x2048x1024 --reps 2
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hipabi as hip  # noqa: E402
import stereo_device as sd  # noqa: E402
import synthetic  # noqa: E402
import tf_checkpoint  # noqa: E402
from model import NET  # noqa: E402

HBM_PEAK = 8.0e12


def shape(s):
    W, H, D = (int(x) for x in s.split("x"))
    return H, W, D


def time_sgm_passes(m, H, W, D, reps):
    """Each direction alone on the left volume of the matcher's workspace (flag planes built once): median ms."""
    ws = m.workspace(H, W, D)
    vol = ws["vol"][0][:H * W * sd.hwd_pitch(D)].view(H, W, sd.hwd_pitch(D))
    g = torch.Generator(device="cuda").manual_seed(1)
    vol.copy_(torch.rand(vol.shape, device="cuda", generator=g))
    L = torch.randn((H, W), device="cuda", generator=g) * 0.07
    R = torch.randn((H, W), device="cuda", generator=g) * 0.07
    flags = sd.sgm_flag_planes(L, R, D, m.hp["sgm_D"], out=ws["sgm_flags"])
    p = [sd._f32(x) for x in (m.hp["sgm_P1"], m.hp["sgm_P2"], m.hp["sgm_Q1"], m.hp["sgm_Q2"])]
    out = {}
    for i, r in enumerate(sd.SGM_DIRECTIONS):
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sd.sgm_pass_flagged_hwd([vol], [hip.MCCNN_SIDE_LEFT], D, r, *p, flags[i])
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[r] = float(np.median(ts[1:]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=["2880x1988x800", "2880x1988x256"], help="WxHxD")
    ap.add_argument("--reps", type=int, default=3, help="timed pairs (and timed passes) per shape, after one warm-up")
    args = ap.parse_args()
    hip.require_device()
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    print("device: %s, %.0f GB" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).total_memory / 1e9))
    for s in args.shapes:
        H, W, D = shape(s)
        dp = sd.hwd_pitch(D)
        vol_gb = H * W * dp * 4 / 1e9
        m = sd.StereoMatcher(net, on_saturation="ignore")
        print("\n== %dx%dx%d: volume %.2f GB (%s 4 GiB), workspace %.2f GB, aggregation: %s" % (
            W, H, D, vol_gb, "past" if H * W * dp * 4 >= 1 << 32 else "below", sd.workspace_bytes(H, W, D) / 1e9,
            "programs" if hip.load().mccnn_cbca_prog_bytes(D, H, W) else "cbca_hwd_kernel"))
        L, R, _, _, _ = synthetic.make_pair(H, W, min(D, 256), seed=100)
        dl, dr = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
        m.match(dl, dr, D)
        torch.cuda.synchronize()
        walls, stages = [], {}
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m.match(dl, dr, D)
            b.record()
            torch.cuda.synchronize()
            walls.append(a.elapsed_time(b))
        timer = sd.StageTimer(True)
        m.match(dl, dr, D, timer=timer)
        torch.cuda.synchronize()
        print("match(): %.1f ms per pair (median of %d, stages overlapped)" % (float(np.median(walls)), len(walls)))
        print("per stage, one pair timed launch by launch (ms):")
        for name, ts in timer.summary_ms().items():
            stages[name] = sum(ts)
            print("  %-28s %9.2f  (%d launches)" % (name, sum(ts), len(ts)))
        for name, ts in timer.spans_ms().items():
            print("  [span] %-21s %9.2f" % (name, max(ts)))
        sg = time_sgm_passes(m, H, W, D, args.reps)
        voxels = H * W * D
        print("SGM, one direction on one volume (median ms; algorithmic 8 B/voxel vs %.0f TB/s):" % (HBM_PEAK / 1e12))
        for r, ms in sg.items():
            bw = 8.0 * voxels / (ms * 1e-3)
            print("  r=%-8s %-10s %8.3f ms  %6.2f TB/s  %5.1f %%" % (
                "(%d,%d)" % r, "horizontal" if r[0] == 0 else "vertical", ms, bw / 1e12, 100 * bw / HBM_PEAK))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
