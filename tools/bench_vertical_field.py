#!/usr/bin/env python3
"""What a field of row offsets costs: writes one JSON object to profiles/vertical_field.json.

    python tools/bench_vertical_field.py [--out profiles/vertical_field.json] [--rounds 5] [--iters 200] [--pair-iters 50]

Every shape is measured by a child process of its own under `timeout -k 10 <--limit seconds>`; the first one that fails
ends the run.  At 750 x 500 x 256 and 1242 x 375 x 228, on the features of a synthetic pair whose right image is rolled
by +-3 rows (tests/vertical_field_reference.py's shear, restated here), all in one process per shape, the launches
alternating leg by leg (HIP events around `iters` launches; the median and the lowest leg of `rounds`):
  - mccnn_cost_volume_hwd (MCCNN_CV_EXACT), time T0, and mccnn_cost_volume_offset_hwd at vertical_range 0, time T1: the
    yardsticks, taken in the same run;
  - mccnn_cost_volume_field_hwd at range 0 on a constant 3 x 4 field and on the 3 x 4 field of the roll, -3 -1 +1 +3
    across; S, the product sets the launch issues, is counted on the host from the field by the kernel's own rule
    (product_sets below restates cvf_tile of csrc/cost_volume.hip);
  - mccnn_vertical_field_select and mccnn_vertical_offset_select on the votes of the (4, 8) profile;
  - the captured pair (match_graph) of a matcher with vertical_offset="grid", of one without, and of a second one
    without: two captures of one pair differ by more than a small kernel takes.
Expectations, each against figures of the same run: the constant field within 1.25 T1; the roll field within
S x T0 x 1.25; the field select within 1.25 x the offset select.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

SHAPES = ((500, 750, 256), (375, 1242, 228))       # (H, W, D)
PROFILE = (4, 8)                                   # (max_offset, row_step)
GRID = (3, 4)
ROLL = (-3, -1, 1, 3)                              # the field of the roll, across; the same in every row band
MARGIN = 1.25
TILE, DTILE, OFFSET_MAX = 63, 64, 8


def product_sets(H, W, D, field, vrange):
    """S: the product sets mccnn_cost_volume_field_hwd issues for this field, in units of one view's whole image - per
    (view, 63-pixel tile, row, 64-disparity tile) one for every candidate row that an entry of the tile selects."""
    gh, gw = len(field), len(field[0])
    nb = (W + 63) // 64
    issued = tiles = 0
    for right in (False, True):
        for h in range(H):
            kmin, kmax = (h - (H - 1), h) if right else (-h, H - 1 - h)
            row = field[h * gh // H]
            for bx in range((W + TILE - 1) // TILE):
                w0 = bx * TILE - 1
                whi = min(w0 + TILE, W - 1)
                d0 = 0
                while d0 < D and w0 + TILE >= d0:
                    clo, chi = max(w0 + 1, d0), whi
                    if right:
                        clo, chi = max(w0 + 1 - min(d0 + DTILE - 1, D - 1), 0), whi - d0
                    xlo, xhi = (W - 1 - chi, W - 1 - clo) if right else (clo, chi)
                    selected = set()
                    if clo <= chi:
                        for blk in range(min(max(xlo, 0), W - 1) // 64, min(max(xhi, 0), W - 1) // 64 + 1):
                            f = min(max(row[min(blk, nb - 1) * gw // nb], -OFFSET_MAX), OFFSET_MAX)
                            lo, hi = max(f - vrange, kmin), min(f + vrange, kmax)
                            if lo > hi:
                                lo = hi = min(max(f, kmin), kmax)
                            selected.update(range(lo, hi + 1))
                    issued += max(1, len(selected))
                    tiles += 1
                    d0 += DTILE
    return 2.0 * issued / tiles


def shear_columns(image, ax):
    """The image rolled by whole rows: pixel (h, x) shows row clip(h - rint(ax (x - cx) / cx), 0, H - 1)."""
    import numpy as np
    H, W = image.shape[:2]
    cx = (W - 1) / 2.0
    dy = np.rint(ax * (np.arange(W) - cx) / cx).astype(np.int64)
    return np.ascontiguousarray(image[np.clip(np.arange(H)[:, None] - dy[None, :], 0, H - 1), np.arange(W)[None, :]])


def measure(shape, args):
    import torch
    import _hipabi as hip
    import stereo_device as sd
    import synthetic
    import tf_checkpoint
    from model import NET

    def leg(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    def alternate(variants, rounds, iters):
        for fn in variants.values():
            leg(fn, max(3, iters // 20))
        legs = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                legs[name].append(leg(fn, iters))
        return {name: dict(median_ms=statistics.median(v), min_ms=min(v), legs_ms=v) for name, v in legs.items()}

    hip.require_device()
    H, W, D = shape
    R, step = PROFILE
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    net.set_layers(tf_checkpoint.load_fast_net_weights(os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")))
    l8, r8, _ = synthetic.make_scene_u8(H, W, D, 100)
    r8 = shear_columns(r8, 3)
    l = torch.from_numpy(synthetic.standardize(l8)[:, :, 0].copy()).cuda()
    r = torch.from_numpy(synthetic.standardize(r8)[:, :, 0].copy()).cuda()
    fl, fr = (t.clone() for t in net.features_pair_hwc_split(l, r))
    out = tuple(torch.zeros((H, W, sd.hwd_pitch(D)), dtype=torch.float32, device="cuda") for _ in range(2))
    grid = sd.vertical_field_grid(H, W, GRID, step)
    assert grid == GRID, grid
    votes = sd.vertical_profile(fl, fr, D, R, step)
    offset, totals = sd.vertical_offset_select(votes, R)
    selected = sd.vertical_field_select(votes, H, step, R, grid)
    measured = sd.vertical_field_record(selected[2].cpu().numpy(), selected[3].cpu().numpy(), selected[0].cpu().numpy(),
                                        selected[1].cpu().numpy())
    zero = torch.zeros((1,), dtype=torch.int32, device="cuda")
    constant = torch.zeros(grid, dtype=torch.int32, device="cuda")
    roll_host = [list(ROLL) for _ in range(grid[0])]
    roll = torch.tensor(roll_host, dtype=torch.int32, device="cuda")
    kernel = alternate({
        "mccnn_cost_volume_hwd": lambda: sd.cost_volume_hwd(fl, fr, D, out=out),
        "offset_range_0": lambda: sd.cost_volume_offset_hwd(fl, fr, D, zero, 0, out=out),
        "field_constant": lambda: sd.cost_volume_field_hwd(fl, fr, D, constant, 0, out=out),
        "field_roll": lambda: sd.cost_volume_field_hwd(fl, fr, D, roll, 0, out=out),
        "offset_select": lambda: sd.vertical_offset_select(votes, R, out=(offset, totals)),
        "field_select": lambda: sd.vertical_field_select(votes, H, step, R, grid, out=selected)},
        args.rounds, args.iters)
    t0, t1 = kernel["mccnn_cost_volume_hwd"]["median_ms"], kernel["offset_range_0"]["median_ms"]
    for v in kernel.values():
        v["times_T0"] = v["median_ms"] / t0
    kernel["field_constant"]["product_sets"] = product_sets(H, W, D, [[0] * grid[1]] * grid[0], 0)
    kernel["field_constant"]["times_T1"] = kernel["field_constant"]["median_ms"] / t1
    s = product_sets(H, W, D, roll_host, 0)
    kernel["field_roll"]["product_sets"] = s
    kernel["field_roll"]["times_T0_per_product_set"] = kernel["field_roll"]["times_T0"] / s
    kernel["field_select"]["times_offset_select"] = kernel["field_select"]["median_ms"] / kernel["offset_select"]["median_ms"]
    expected = dict(constant_field_within_1p25_T1=kernel["field_constant"]["times_T1"] <= MARGIN,
                    roll_field_within_S_x_T0_x_1p25=kernel["field_roll"]["times_T0"] <= s * MARGIN,
                    field_select_within_1p25_offset_select=kernel["field_select"]["times_offset_select"] <= MARGIN)
    del fl, fr, out, votes
    torch.cuda.empty_cache()
    plain = sd.StereoMatcher(net, on_saturation="ignore")
    field = sd.StereoMatcher(net, on_saturation="ignore", extras=dict(vertical_offset="grid", vertical_offset_grid=GRID,
                                                                      vertical_offset_max=R, vertical_offset_rows=step))
    again = sd.StereoMatcher(net, on_saturation="ignore")
    pair = alternate({"pair": lambda: plain.match_graph(l, r, D), "pair_grid": lambda: field.match_graph(l, r, D),
                      "pair_again": lambda: again.match_graph(l, r, D)}, args.rounds, args.pair_iters)
    pair["report"] = field.vertical_report(H, W, D)
    pair["added_ms"] = pair["pair_grid"]["median_ms"] - pair["pair"]["median_ms"]
    pair["spread_of_two_captures_ms"] = abs(pair["pair_again"]["median_ms"] - pair["pair"]["median_ms"])
    print("%dx%dx%d  T0 %.4f ms, T1 %.4f ms; constant field %.2f x T1; roll field %.2f x T0 at S = %.2f; select %.4f ms "
          "(offset select %.4f ms); measured %s; pair %.3f -> %.3f ms with 'grid' (a second plain matcher: %.3f)" % (
              W, H, D, t0, t1, kernel["field_constant"]["times_T1"], kernel["field_roll"]["times_T0"], s,
              kernel["field_select"]["median_ms"], kernel["offset_select"]["median_ms"], measured["offsets"],
              pair["pair"]["median_ms"], pair["pair_grid"]["median_ms"], pair["pair_again"]["median_ms"]), flush=True)
    return dict(device=torch.cuda.get_device_name(0), T0_ms=t0, T1_ms=t1, measured=measured, kernel=kernel,
                expected=expected, captured_pair=pair)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_field.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pair-iters", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds one shape's process may take")
    ap.add_argument("--shape", type=int, default=None, help="(the child's) index into SHAPES; its result goes to --out")
    args = ap.parse_args()
    if args.shape is not None:
        with open(args.out, "w") as f:
            json.dump(measure(SHAPES[args.shape], args), f)
        return 0
    result = dict(rounds=args.rounds, iters=args.iters, pair_iters=args.pair_iters, margin=MARGIN, profile=list(PROFILE),
                  grid=list(GRID), roll=list(ROLL), shapes={})
    for i, (H, W, D) in enumerate(SHAPES):
        part = "%s.part%d" % (args.out, i)
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--shape",
                              str(i), "--out", part, "--rounds", str(args.rounds), "--iters", str(args.iters),
                              "--pair-iters", str(args.pair_iters)])
        if rc != 0:
            print("%dx%dx%d: the child ended with status %d; nothing further is started" % (W, H, D, rc), file=sys.stderr)
            return rc
        with open(part) as f:
            shape = json.load(f)
        os.remove(part)
        result["device"] = shape.pop("device")
        result["shapes"]["%dx%dx%d" % (W, H, D)] = shape
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
