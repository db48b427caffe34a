#!/usr/bin/env python3
"""Benchmark of the stereo-matching hot path (the timed region of the reference's match.py:129-179).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2] [--fast] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-parity] [--no-bounds]]

The benchmarked variant is the drop-in default of match.py: float32 throughout, every stage behind the conv features
bit-identical to the reference's NumPy (`--fast` selects the tolerance-checked variants instead; their stated tolerance
lives in src/tolerances.py).

A plain run sets up, warms up, times K pairs and prints the headline line (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, ...).  `--dump-outputs DIR` also writes the final disparity map of the last
timed step as DIR/disparity.npy (float32; rank r > 0: DIR/disparity_rank<r>.npy); the inputs are seeded, so two builds
can be compared output for output.  `--full` adds everything else to the line: a `parity` block measured on the very
pair that was timed (the script then EXITS NON-ZERO when that block violates what `config.variant` states), the other
variant's time, per-stage times and rooflines, the side measurements and the CPU baseline.

`--gpus N` with N > 1 may be started either by `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`
(one rank per GPU, as the driver does) or directly as `python bench.py --gpus N ...`: without a WORLD_SIZE in the
environment the script re-launches itself under torch.distributed.run on 127.0.0.1.

A step = one stereo pair pushed through features -> cost volume -> CBCA x2 -> SGM (4 directions x 2 volumes)
-> CBCA x16 -> WTA -> LR check/interpolation -> sub-pixel -> median -> bilateral, with the standardised images and the
network weights already resident in HBM.  Metric: Mdisparities/s = H*W*D / seconds (BASELINE.json).  With N > 1
every rank matches its own pair (pairs are the independent unit; no data-path collective) and rank 0 reports the
aggregate over the slowest rank's time (weak scaling).  One JSON line is printed by rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

CONFIGS = {  # BASELINE.json configs: (H, W, D)
    "cfg1": (256, 256, 64),
    "cfg2": (500, 750, 256),     # Middlebury-v3 half-res: the configuration the metric is quoted on
    "cfg3": (375, 1242, 192),    # KITTI-2015
    "cfg4": (1000, 1500, 400),   # Middlebury-v3 full-res
}
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense f16 / bf16 matrix peak, same guide (the headline figures with 2:1 sparsity are not used)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0,
                    help="timed pairs (0 = as many as make the timed region about 3 s: 200 at cfg2, at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--fast", action="store_true",
                    help="the tolerance-checked variant: the cost volume on the matrix cores (split-f16 operands, <= 2e-6) in "
                         "front of the bit-exact stages, instead of the bit-exact float32 default")
    ap.add_argument("--separable-cbca", action="store_true",
                    help="with --fast: also the separable float64-prefix aggregation on plane-major volumes (the fast "
                         "variants of rounds 2-3; slower than the default since round 4)")
    ap.add_argument("--exact", action="store_true", help="(default; kept for older command lines)")
    ap.add_argument("--split-features", action="store_true", help="(default; kept for older command lines)")
    ap.add_argument("--library-features", action="store_true",
                    help="conv features through the float32 library convolutions (MIOpen) instead of the hand-written "
                         "split-operand matrix-core kernels (which are as close to a float64 evaluation as the library)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the final disparity map of the last timed step to DIR/disparity.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the parity block (exit 3 on a violation), the other variant, per-stage "
                         "times and rooflines, the side measurements and the CPU baseline (the --no-* options below "
                         "switch parts of it off)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true",
                    help="skip the parity block (graph replay vs eager, benchmarked variant vs the bit-exact variant)")
    ap.add_argument("--no-bounds", action="store_true",
                    help="skip the content-independence side measurements (the same pair without skipping, the worst-case "
                         "scene) and the library-feature timing: under rocprofv3 every launch of a kernel then belongs to "
                         "the benchmarked pair, so the table's averages are comparable with the line's per-launch events")
    ap.add_argument("--no-graph", action="store_true",
                    help="launch the ~75 kernels of a pair one by one instead of replaying the captured hipGraph")
    ap.add_argument("--cpu-sample", default="auto",
                    help="what every CPU-baseline worker runs: `auto` = a full-width row window of the benchmarked "
                         "workload sized for ~25 s per worker (cfg2: 36 rows x 750 x 256), a BASELINE config name (one "
                         "whole pair; cfg2 takes ~6 min per core), or an HxW window of the benchmarked workload")
    ap.add_argument("--cpu-cores", type=int, default=0,
                    help="CPU-baseline worker processes (0 = half of the host threads, at most 16)")
    a = ap.parse_args()
    if a.fast and a.exact:
        ap.error("--fast and --exact exclude each other")
    if a.separable_cbca and not a.fast:
        ap.error("--separable-cbca belongs to --fast")
    a.exact = not a.fast
    return a


def cpu_baseline(H, W, D, sample, cores, wpath):
    """The oracle (a scalar C port of the reference's loops, oracle/mccnn_oracle.c) timed on the host: `cores` worker
    processes (oracle/cpu_window.py) started together, each pushing one full-width row window of the benchmarked
    workload (default; every worker its own synthetic window, same width and disparity range as the GPU's pair) - or
    ONE whole stereo pair of a BASELINE config - through the complete timed region; the rate is all their voxels over
    the slowest worker's time.  Reported next to the GPU number; never on the measured path.  A whole cfg2 pair on
    one core is run once per round and kept under profiles/ (it takes ~6 minutes)."""
    import subprocess
    if sample == "auto":
        sample = "%dx%d" % (max(32, min(H, int(round(7.0e6 / (W * D))))), W)
    if sample in CONFIGS:
        sh, sw, sd_ = CONFIGS[sample]
        what = "one whole %s pair (%dx%d, D=%d)" % (sample, sw, sh, sd_)
    else:
        sh, sw = [int(x) for x in sample.split("x")]
        sh, sw, sd_ = min(sh, H), min(max(sw, D + 2), W), D
        what = "one %dx%d window, D=%d (%.1f%% of the %dx%d workload)" % (sw, sh, sd_, 100.0 * sh * sw / (H * W), W, H)
    worker = os.path.join(ROOT, "oracle", "cpu_window.py")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    t0 = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, worker, str(sh), str(sw), str(sd_), str(1 + i), wpath],
                              stdout=subprocess.PIPE, env=env) for i in range(cores)]
    secs = []
    for p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("cpu_baseline worker failed")
        secs.append(float(out.decode().strip().splitlines()[-1]))
    wall = time.perf_counter() - t0
    slowest = max(secs)
    return {"value": round(cores * sh * sw * sd_ / slowest / 1e6, 5), "unit": "Mdisparities/s", "cores": cores,
            "kind": "port",
            "sample": "%d workers x %s each, whole timed region incl. the conv stack; slowest %.1f s, fastest %.1f s "
                      "(%.3f Mdisp/s per core), %.0f s wall on %d host threads; the reference's own interpreted "
                      "loops measured 0.0068 Mdisp/s on one core (BASELINE.md)"
                      % (cores, what, slowest, min(secs), sh * sw * sd_ / min(secs) / 1e6, wall, os.cpu_count() or 0)}


def run_host_io(matcher, host_left, host_right, D, use_graph):
    """One pair the way match.py:129-179 times it: standardised host images in, host disparity map out."""
    dl = host_left.cuda(non_blocking=True)
    dr = host_right.cuda(non_blocking=True)
    out = matcher.match_graph(dl, dr, D) if use_graph else matcher.match(dl, dr, D)
    return out.cpu()


def traffic_table(config):
    """HBM-side bytes per launch from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json): they cannot be
    counted live.  An entry is used only when it was taken on this workload AND the kernel source it names still has
    the hash recorded with it - otherwise the kernel has changed since it was profiled and traffic is null."""
    import hashlib
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.isfile(tpath):
        return {}
    with open(tpath) as f:
        tj = json.load(f)
    if tj.get("workload") != config:
        return {}
    out = {}
    for k, v in tj.items():
        if not isinstance(v, dict) or "traffic_bytes" not in v:
            continue
        src = os.path.join(ROOT, v.get("source", ""))
        if not os.path.isfile(src):
            continue
        with open(src, "rb") as f:
            if hashlib.sha256(f.read()).hexdigest()[:16] != v.get("source_sha256_16"):
                continue
        out[k] = {"bytes": int(v["traffic_bytes"]), "from": v.get("profile")}
    return out


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started bare: become the launcher (one rank per GPU over RCCL, rendezvous on the loopback address)
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.stdout.flush()
        os.execv(sys.executable, cmd)

    import numpy as np
    import torch

    import _hipabi as hip
    import distributed as mgpu
    import stereo_device as sd
    import synthetic
    import tf_checkpoint
    from model import NET

    hip.require_device()  # raises without a GPU or without the built library: no fallback
    # MCCNN_BENCH_SHARED_GPU=1 (tests only): ranks share the visible GPUs round-robin and rendezvous over gloo, so the
    # N > 1 control flow of this file can run on a one-GPU box; RCCL refuses two ranks on one device
    shared = os.environ.get("MCCNN_BENCH_SHARED_GPU") == "1"
    device_index = local_rank % torch.cuda.device_count() if shared else local_rank
    torch.cuda.set_device(device_index)
    # MCCNN_BENCH_FORCE_DIST=1 (tests): join a process group even at world size 1, so that the RCCL initialisation,
    # barrier and all_gather of the multi-GPU path run on a one-GPU box
    force = os.environ.get("MCCNN_BENCH_FORCE_DIST") == "1"
    if shared:
        mgpu.init("gloo", always=force)
    else:
        mgpu.init("nccl", torch.device("cuda", device_index), always=force)   # RCCL: barrier + timing all_gather only

    H, W, D = CONFIGS[args.config]
    if args.steps <= 0:      # ~3 s of timed region: 14 ms per cfg2 pair -> 200 steps (the same count on every rank)
        args.steps = max(20, int(round(200.0 * 96.0e6 / (H * W * D))))
    wpath = os.path.join(ROOT, "tests", "golden", "mccnn_fast_weights.npz")
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=0)
    layers = None
    if os.path.isfile(wpath):
        layers = tf_checkpoint.load_fast_net_weights(wpath)
        net.set_layers(layers)
    else:
        layers = net.get_layers()
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100 + rank)   # every rank owns a different pair
    dl = torch.from_numpy(L[:, :, 0]).cuda()
    dr = torch.from_numpy(R[:, :, 0]).cuda()
    lib_features = args.library_features
    matcher = sd.StereoMatcher(
        net, cv_mode=hip.MCCNN_CV_EXACT if args.exact else hip.MCCNN_CV_MFMA,
        cbca_order=hip.MCCNN_CBCA_SEPARABLE if args.separable_cbca else hip.MCCNN_CBCA_REFERENCE_ORDER,
        features="miopen" if lib_features else "split_f16",
        on_saturation="ignore")      # nothing may block inside the timed loop: the flag is read once, in `parity`

    use_graph = not args.no_graph
    if use_graph:
        try:                                     # the first call warms up eagerly, then captures
            matcher.match_graph(dl, dr, D)
            torch.cuda.synchronize()
        except Exception as e:                   # capture refused (e.g. a library call that cannot be captured):
            sys.stderr.write("bench: hipGraph capture failed (%s); launching kernel by kernel\n" % e)   # still the HIP path
            use_graph = False
            torch.cuda.synchronize()
    run = (lambda: matcher.match_graph(dl, dr, D)) if use_graph else (lambda: matcher.match(dl, dr, D))
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    mgpu.barrier()
    # headline loop: nothing but K pairs between the two synchronisation points (no per-stage events in here)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = run()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    mgpu.barrier()
    if args.dump_outputs:
        # what the timed path handed its caller in the last step: the final disparity map [H, W], float32
        os.makedirs(args.dump_outputs, exist_ok=True)
        name = "disparity.npy" if rank == 0 else "disparity_rank%d.npy" % rank
        np.save(os.path.join(args.dump_outputs, name), out.cpu().numpy().astype(np.float32))

    all_elapsed = mgpu.gather_elapsed(elapsed)
    elapsed_max = max(all_elapsed)
    props = torch.cuda.get_device_properties(device_index)
    devices = mgpu.gather_objects({"rank": rank, "local_rank": local_rank, "device": device_index, "name": props.name,
                                   "visible": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES")),
                                   "pci_bus_id": getattr(props, "pci_bus_id", None), "cus": props.multi_processor_count})
    if rank != 0:
        mgpu.finalize()
        return

    voxels = H * W * D
    value = world * voxels * args.steps / elapsed_max / 1e6
    result = {
        "metric": "Mdisparities/s (HxWxD / s) end-to-end match.py timed region, images resident in HBM",
        "value": round(value, 2), "unit": "Mdisparities/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed_max / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.exact else
        "f32 (split-f16 operands: 22-bit products, float32 accumulate, in the cost volume)",
        "data": "synthetic",
        "config": {"workload": "%s: %dx%d synthetic stereo pair, D=%d, one pair per GPU" % (args.config, W, H, D),
                   "variant": "bit-exact (float32; every stage after the conv features bit-identical to the reference's "
                              "NumPy on the same features; the features within 3e-7 of a float64 evaluation of the network)"
                   if args.exact else
                   "fast (split-f16 MFMA cost volume%s); stated tolerance against the "
                   "bit-exact variant (src/tolerances.py, asserted on `parity` under --full): WTA flips <= 1e-4 of the "
                   "pixels per view, >= 98 %% of the final map within 1e-3 px, 99th percentile <= 0.02 px"
                   % (", separable float64-prefix CBCA on plane-major volumes" if args.separable_cbca
                      else " in front of the bit-exact stages"),
                   "features": "float32 library convolutions (MIOpen)" if lib_features else
                   "hand-written matrix-core convolutions (float32 in/out; every operand as two f16 parts, 3 products per "
                   "multiply, float32 accumulation with the cross terms in their own accumulator: 2.6e-7 .. 3.1e-7 from a "
                   "float64 evaluation where the library path is 2.7e-7 .. 2.8e-7, profiles/parity_features_split_r04.json)",
                   "launch": ("one hipGraph replay per pair" if use_graph else "kernel by kernel") +
                   ("; each volume's aggregation -> SGM -> aggregation is one free-running chain of one-volume launches "
                    "on its own stream (StereoMatcher's default since round 6), joined in front of the WTA-carrying "
                    "last aggregation launch" if (matcher.free_chains and matcher.two_chains and matcher.pixel_major()) else ""),
                   "weights": "converted reference checkpoint" if os.path.isfile(wpath) else "random init"},
    }
    ranks = {
        "per_rank_ms_per_step": [round(e / args.steps * 1e3, 3) for e in all_elapsed],
        "per_rank_device": devices,
        "process_group": (torch.distributed.get_backend() + " x%d" % torch.distributed.get_world_size())
        if torch.distributed.is_initialized() else None,
    }
    if not args.full:
        # the plain run: the headline and nothing else (no parity, side measurements, rooflines or CPU baseline)
        result.update(ranks)
        print(json.dumps(result))
        mgpu.finalize()
        return

    # ---- parity of what was just timed (rank 0, outside the timed region) -------------------------------------------
    # (1) the replayed graph against the same matcher launched kernel by kernel: bit-identical or the capture is wrong;
    # (2) the benchmarked variant against the bit-exact variant on this very pair: WTA flips and final-map distance.
    #     The bit-exact variant is pinned stage by stage against the CPU oracle / the reference's golden vectors by the
    #     test-suite (cfg1 whole pair, ragged shapes); at this size it is the proxy for the reference.  When the
    #     benchmarked variant IS the bit-exact one, it is cross-checked against its plane-major twin (the round-2
    #     reference-order kernels on [D,H,W]), which must agree bit for bit.
    parity, other_ms, other_parity, violations = None, None, None, []
    is_default = args.exact                           # the drop-in default: float32, bit-exact behind the features

    def compare(out_a, keep_a, out_b, keep_b):
        """Distance of two final maps / WTA maps (NaN == NaN; inf where only one side is finite)."""
        both_nan = torch.isnan(out_a) & torch.isnan(out_b)
        diff = torch.where(both_nan, torch.zeros_like(out_a), (out_a - out_b).abs())
        diff = torch.nan_to_num(diff, nan=float("inf"), posinf=float("inf"))
        finite = torch.isfinite(diff)
        k99, k = max(1, int(round(0.99 * diff.numel()))), max(1, int(round(0.999 * diff.numel())))
        return {
            "pixels": H * W,
            "wta_flips_left": int((keep_a["wta"][0] != keep_b["wta"][0]).sum()),
            "wta_flips_right": int((keep_a["wta"][1] != keep_b["wta"][1]).sum()),
            "frac_within_1e-3_px": round(float((diff <= 1e-3).float().mean()), 6),
            "p99_abs_px": round(float(diff.flatten().kthvalue(k99).values), 6),
            "p99.9_abs_px": round(float(diff.flatten().kthvalue(k).values), 6),
            "max_abs_px": round(float(diff[finite].max()) if bool(finite.any()) else 0.0, 6),
            "final_map_bit_identical": bool(torch.equal(out_a.contiguous().view(torch.int32),
                                                        out_b.contiguous().view(torch.int32))),
        }

    def timed(m, n, a=None, b=None):
        a, b = (dl, dr) if a is None else (a, b)
        try:
            m.match_graph(a, b, D)
            go = lambda: m.match_graph(a, b, D)          # noqa: E731
        except Exception:
            go = lambda: m.match(a, b, D)                # noqa: E731
        go()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            go()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    if not args.no_parity:
        import tolerances as tol
        out_timed = out.clone()
        keep_b = {}
        out_eager = matcher.match(dl, dr, D, keep=keep_b)
        torch.cuda.synchronize()
        same_as_eager = bool(torch.equal(out_timed.view(torch.int32), out_eager.view(torch.int32)))
        if not same_as_eager:
            violations.append("the replayed graph differs from the kernel-by-kernel launch")
        if matcher.features == "split_f16" and matcher.features_saturated():
            violations.append("an activation left the range of the split-operand feature records")
        if is_default:
            # the benchmarked variant IS the bit-exact one: cross-checked against its plane-major twin (the round-2
            # reference-order kernels on [D,H,W]; same feature kernels), which is pinned stage by stage against the CPU
            # oracle and the reference's golden vectors by the test-suite; the two must agree bit for bit
            ref = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER,
                                   features=matcher.features, layout="plane_major")
            ref_name = "the same variant on plane-major volumes (round-2 reference-order kernels, pinned to the oracle)"
        else:
            ref = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
            ref_name = "bit-exact variant (NumPy-order cost volume, reference-order CBCA; the same feature kernels)"
        keep_e = {}
        out_ref = ref.match(dl, dr, D, keep=keep_e)
        torch.cuda.synchronize()
        parity = dict({"timed_path_equals_kernel_by_kernel": same_as_eager, "against": ref_name},
                      **compare(out_eager, keep_b, out_ref, keep_e))
        if is_default:
            if not parity["final_map_bit_identical"] or parity["wta_flips_left"] or parity["wta_flips_right"]:
                violations.append("the bit-exact variant differs from its plane-major twin")
        else:
            violations += tol.fast_violations(H * W, parity["wta_flips_left"], parity["wta_flips_right"],
                                              parity["frac_within_1e-3_px"], parity["p99_abs_px"])
        del ref
        # the other variant on the same box and pair, outside `value` (10 pairs, graph replay): the fast variants when
        # the default was benchmarked (with their distance to it), the default when a fast variant was
        if is_default:
            other = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER,
                                     features="split_f16")
            keep_o = {}
            out_o = other.match(dl, dr, D, keep=keep_o)
            torch.cuda.synchronize()
            other_parity = compare(out_o, keep_o, out_eager, keep_b)
            other_parity["stated"] = {"wta_flip_fraction": tol.FAST_WTA_FLIP_FRACTION,
                                      "frac_within_1e-3_px": tol.FAST_FRAC_WITHIN_1E3_PX,
                                      "p99_abs_px": tol.FAST_P99_ABS_PX}
            other_parity["violations"] = tol.fast_violations(H * W, other_parity["wta_flips_left"],
                                                             other_parity["wta_flips_right"],
                                                             other_parity["frac_within_1e-3_px"],
                                                             other_parity["p99_abs_px"])
            del keep_o
        else:
            other = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
        del keep_b, keep_e
        other_ms = timed(other, 10)
        del other

    # side measurements on rank 0, outside the reported number
    nside = max(2, min(args.steps, 5))
    timer = sd.StageTimer(True)                  # per-launch HIP events, launches issued one by one
    matcher.match(dl, dr, D)
    torch.cuda.synchronize()
    for _ in range(nside):
        matcher.match(dl, dr, D, timer=timer)
    torch.cuda.synchronize()
    t1 = time.perf_counter()                     # launches one by one, no events
    for _ in range(nside):
        matcher.match(dl, dr, D)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t1) / nside * 1e3
    lib_ms = None
    if matcher.features != "miopen" and not args.no_bounds:   # the same pair with the float32 library convolutions, for reference
        mlib = sd.StereoMatcher(net, cv_mode=matcher.cv_mode, cbca_order=matcher.cbca_order, features="miopen")
        mlib._ws = matcher._ws                   # same shape: shares the resident workspace
        mlib.match(dl, dr, D)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for _ in range(nside):
            mlib.match(dl, dr, D)
        torch.cuda.synchronize()
        lib_ms = (time.perf_counter() - t3) / nside * 1e3
    # How much of the headline is a property of THIS image?  (a) the same pair with every aggregation iteration on the
    # full programs (no pixel is skipped): what the kernels cost when no support region is a single pixel; (b) the
    # second seeded scene class - the flat blobs without the texture half (synthetic.make_pair(texture=False)): a few
    # per cent of unit-region pixels, support regions of several hundred pixels almost everywhere, i.e. the reference's
    # running sums (pf:157-161) at their longest: the aggregation is then bound by its additions, not by bytes.
    noskip_ms = worst_ms = worst_unit = joined_ms = natural_ms = natural_unit = None
    in_flight = {}
    if not args.no_bounds and matcher.pixel_major() and matcher.workspace(H, W, D)["progs"] is not None:
        # round 5's launch structure (StereoMatcher(free_chains=False)): the two chains of one-volume aggregation launches
        # join after every stage and the SGM passes are two-volume launches; same bits
        m4 = sd.StereoMatcher(net, cv_mode=matcher.cv_mode, cbca_order=matcher.cbca_order, features=matcher.features,
                              on_saturation="ignore", free_chains=False)
        m4._ws = matcher._ws
        joined_ms = timed(m4, 10)
        del m4
        m2 = sd.StereoMatcher(net, cv_mode=matcher.cv_mode, cbca_order=matcher.cbca_order, features=matcher.features,
                              on_saturation="ignore", skip_unit_regions=False)
        m2._ws = matcher._ws
        noskip_ms = timed(m2, 10)
        del m2
        Lw, Rw, _, _, _ = synthetic.make_pair(H, W, D, seed=100 + rank, texture=False)
        dlw, drw = torch.from_numpy(Lw[:, :, 0]).cuda(), torch.from_numpy(Rw[:, :, 0]).cuda()
        m3 = sd.StereoMatcher(net, cv_mode=matcher.cv_mode, cbca_order=matcher.cbca_order, features=matcher.features,
                              on_saturation="ignore")
        m3._ws = matcher._ws
        worst_ms = timed(m3, 3, dlw, drw)
        wsw = m3.workspace(H, W, D)
        worst_unit = {k2: round(float(((wsw[k] & 0xfffff) == 0).float().mean().item()), 4)
                      for k, k2 in (("sup_l", "left"), ("sup_r", "right"))}
        # (c) the third seeded scene class - synthetic.make_pair(kind="natural"): a 1/f amplitude spectrum, 8 bit,
        # standardised like match.py:120-121 - i.e. the second-order statistics of a photograph: the arm threshold is
        # about one grey level, almost every support region is the pixel itself and the skip launches are almost empty
        Ln, Rn, _, _, _ = synthetic.make_pair(H, W, D, seed=100 + rank, kind="natural")
        dln, drn = torch.from_numpy(Ln[:, :, 0]).cuda(), torch.from_numpy(Rn[:, :, 0]).cuda()
        natural_ms = timed(m3, 10, dln, drn)
        natural_unit = {k2: round(float(((wsw[k] & 0xfffff) == 0).float().mean().item()), 4)
                        for k, k2 in (("sup_l", "left"), ("sup_r", "right"))}
        del m3
        matcher.match(dl, dr, D)                 # the shared workspace holds the benchmark pair's arms again
        torch.cuda.synchronize()
        # Throughput with several pairs in flight - the reference's own scheme is several match.py processes with
        # different -s/-e windows on one GPU (match.py:26-28): N matchers, each with its own workspace, streams and
        # captured graph, replayed round-robin on N streams.  Outside `value` (the headline stays one pair per GPU).
        for n_fl in (2, 4):
            free_b, _total_b = torch.cuda.mem_get_info()
            need = n_fl * 6.5 * 4.0 * H * W * D                        # ~4 volumes + programs + conv activations each
            if need > 0.8 * free_b:
                continue
            ms_ = [sd.StereoMatcher(net, cv_mode=matcher.cv_mode, cbca_order=matcher.cbca_order, features=matcher.features,
                                    on_saturation="ignore") for _ in range(n_fl)]
            sts = [torch.cuda.Stream() for _ in range(n_fl)]
            try:
                for m_, st_ in zip(ms_, sts):
                    with torch.cuda.stream(st_):
                        m_.match_graph(dl, dr, D)
                        m_.match_graph(dl, dr, D)
                torch.cuda.synchronize()
                npairs = 12 * n_fl
                t4 = time.perf_counter()
                for i in range(npairs):
                    with torch.cuda.stream(sts[i % n_fl]):
                        last_ = ms_[i % n_fl].match_graph(dl, dr, D)
                torch.cuda.synchronize()
                in_flight[n_fl] = {"ms_per_pair": round((time.perf_counter() - t4) / npairs * 1e3, 3),
                                   "final_map_equals_the_timed_pair": bool(torch.equal(last_.view(torch.int32),
                                                                                       out.view(torch.int32)))}
            except Exception as e:                                     # e.g. capture refused beside another graph
                in_flight[n_fl] = {"error": str(e)[:200]}
            del ms_, sts
            torch.cuda.empty_cache()
    hl, hr = torch.from_numpy(L[:, :, 0].copy()).pin_memory(), torch.from_numpy(R[:, :, 0].copy()).pin_memory()
    t2 = time.perf_counter()                     # match.py's own region: host images in, host map out
    for _ in range(nside):
        res = run_host_io(matcher, hl, hr, D, use_graph)
    host_io_ms = (time.perf_counter() - t2) / nside * 1e3
    del res

    stages = {k: float(np.mean(v)) for k, v in timer.summary_ms().items()}          # mean ms per launch / stage
    counts = {k: len(v) // nside for k, v in timer.summary_ms().items()}
    # One-volume launches run as two concurrent chains (left volume on the main stream, right volume on a second one):
    # their per-launch durations overlap pairwise in wall time, so a step is charged half of their sum.
    CONCURRENT = ("cbca_iter_prog", "cbca_iter_prog_skip", "sgm_pass_one_volume")
    per_step = {k: stages[k] * counts[k] * (0.5 if k in CONCURRENT else 1.0) for k in stages}     # ms per step
    vol_bytes = 4.0 * voxels
    # algorithmic bytes per launch (SURVEY 8d / DESIGN.md): one read + one write of every voxel the launch owns
    algo = {
        "cbca_iter": 2 * vol_bytes,       # one iteration on one volume
        "cbca_iter_pair": 2 * 2 * vol_bytes,   # one iteration on BOTH volumes (one launch: left + right)
        "cbca_iter_hwd_pair": 2 * 2 * vol_bytes,   # the same, reference-order kernel on pixel-major volumes
        "cbca_iter_prog_pair": 2 * 2 * vol_bytes,  # the same, program-driven assembly kernel (the default)
        "cbca_iter_prog": 2 * vol_bytes,           # ... one volume per launch (two chains of launches on two streams)
        "sgm_pass": 2 * 2 * vol_bytes,    # one direction on BOTH volumes (one launch advances left + right)
        "sgm_pass_one_volume": 2 * vol_bytes,      # one direction on ONE volume (the free-running chains)
        "sgm_first_pass": 2 * 2 * vol_bytes,
    }
    # Iterations 2.. of an aggregation leave the pixels alone whose support region is the pixel itself (their value is
    # a fixed point: mccnn_cbca_iter_prog_pair_skip, include/mccnn.h).  SURVEY 8d prices a CBCA iteration at 8 B per
    # voxel and volume whatever the implementation avoids ("a cache-resident CBCA may legitimately exceed 100 %; report
    # rocprof HBM bytes alongside"): so does `algorithmic_bytes_per_launch`; the entry also carries the stricter figure
    # on the voxels such a launch actually processes, counted from the support planes of the timed pair.
    unit_fraction = None
    algo["cbca_iter_prog_pair_skip"] = 2 * 2 * vol_bytes
    algo["cbca_iter_prog_skip"] = 2 * vol_bytes
    if "cbca_iter_prog_pair_skip" in stages or "cbca_iter_prog_skip" in stages:
        ws = matcher.workspace(H, W, D)
        unit = [float(((ws[k] & 0xfffff) == 0).float().mean().item()) for k in ("sup_l", "sup_r")]
        unit_fraction = {"left": round(unit[0], 4), "right": round(unit[1], 4)}
    traffic = traffic_table(args.config)
    rooflines = {}
    for k, b in algo.items():
        if k in stages:
            ach = b / (stages[k] * 1e-3) / 1e9
            rooflines[k] = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(ach / HBM_PEAK_GBS, 4),
                            "traffic": traffic[k]["bytes"] if k in traffic else None,
                            "traffic_from": traffic[k]["from"] if k in traffic else None,
                            "launches_per_step": counts[k], "avg_launch_ms": round(stages[k], 4),
                            "algorithmic_bytes_per_launch": int(b)}
    for skip_key, volumes in (("cbca_iter_prog_pair_skip", 2), ("cbca_iter_prog_skip", 1)):
        if unit_fraction is None or skip_key not in rooflines:
            continue
        # the units such a launch processes are the voxels of the pixels that are NOT fixed points: `achieved` / `frac`
        # price those (8 B each); the nominal figure on every voxel of the launch's volume(s) is kept beside them
        # (one-volume launches: the mean of the left and the right volume's launches)
        r = rooflines[skip_key]
        processed = 2 * vol_bytes * ((1.0 - unit[0]) + (1.0 - unit[1])) * (volumes / 2.0)
        r["unit_region_pixels"] = unit_fraction
        r["achieved_nominal_8B_per_voxel"], r["frac_nominal_8B_per_voxel"] = r["achieved"], r["frac"]
        r["nominal_bytes_per_launch"] = r["algorithmic_bytes_per_launch"]
        r["algorithmic_bytes_per_launch"] = r["processed_voxel_bytes_per_launch"] = int(processed)
        r["achieved"] = round(processed / (stages[skip_key] * 1e-3) / 1e9, 1)
        r["frac"] = r["frac_on_processed_voxels"] = round(r["achieved"] / HBM_PEAK_GBS, 4)
        r["note"] = ("second and later iterations of an aggregation (not the last, which carries the WTA): pixels whose support region is the pixel itself are "
                     "fixed points and are neither read for their own sake nor written (same bits); algorithmic bytes = "
                     "8 B x the voxels of the OTHER pixels (the units this launch processes), `frac_nominal_8B_per_voxel` "
                     "prices every voxel of the launch as SURVEY 8d words it, `traffic` = the HBM bytes rocprofv3 counted")
    # One-volume launches run as two concurrent chains (left volume on the main stream, right volume on a second one):
    # a launch's duration - by the events on its own stream, and in rocprofv3's table - is its duration WHILE ITS TWIN
    # RUNS, so the per-launch figure is that of a kernel with half of the chip; the aggregation as a stage is priced
    # from the bracket around the whole stage below (`aggregation_stages`).
    for k in CONCURRENT:
        if k in rooflines:
            r = rooflines[k]
            r["concurrent_launches"] = 2
            r["achieved_one_launch"], r["frac_one_launch"] = r["achieved"], r["frac"]
            r["achieved"], r["frac"] = round(2 * r["achieved"], 1), round(2 * r["frac"], 4)
            for kk in ("achieved_nominal_8B_per_voxel", "frac_nominal_8B_per_voxel"):
                if kk in r:
                    r[kk + "_one_launch"] = r[kk]
                    r[kk] = round(2 * r[kk], 4 if kk.startswith("frac") else 1)
            r["frac_on_processed_voxels"] = r["frac"] if "frac_on_processed_voxels" in r else None
            r["concurrency_note"] = ("TWO launches of this kernel run at the same time, one per volume on two streams: "
                                     "`avg_launch_ms` is one launch's duration beside its twin (rocprofv3's table shows the "
                                     "same), `algorithmic_bytes_per_launch` one launch's bytes; `achieved` / `frac` are "
                                     "what the two concurrent launches move together (2 x bytes / avg_launch_ms), "
                                     "`*_one_launch` the same for a single launch; `aggregation_stages` prices the whole "
                                     "stage from a bracket around it and agrees")
    agg_stages = {}
    spans = {k: float(np.mean(v)) for k, v in timer.spans_ms().items()}
    hp_ = matcher.hp
    for name, n_it in (("aggregation_1", int(hp_["cbca_num_iterations1"])), ("aggregation_2", int(hp_["cbca_num_iterations2"]))):
        if name in spans and n_it > 0:
            # stereo_device.cbca_prog_pair's rule for which iterations leave the unit-region pixels alone
            fuse = name == "aggregation_2" and D <= sd.cbca_hwd_wta_max_d()
            n_skip = 0
            if unit_fraction is not None and matcher.skip_unit_regions:
                n_skip = sd.skip_schedule(n_it, fuse, True, matcher.refresh_first).count("skip")
            proc = (n_it - n_skip) * 4 * vol_bytes
            if n_skip:
                proc += n_skip * 2 * vol_bytes * ((1.0 - unit[0]) + (1.0 - unit[1]))
            t = spans[name] * 1e-3
            agg_stages[name] = {"ms": round(spans[name], 4), "iterations": n_it, "skip_iterations": n_skip,
                                "ms_per_iteration": round(spans[name] / n_it, 4),
                                "processed_voxel_bytes": int(proc), "achieved_GBs": round(proc / t / 1e9, 1),
                                "frac_of_hbm_peak": round(proc / t / 1e9 / HBM_PEAK_GBS, 4),
                                "nominal_frac_8B_per_voxel": round(n_it * 4 * vol_bytes / t / 1e9 / HBM_PEAK_GBS, 4)}
    # the conv stack on the matrix cores (north_star: MFMA utilisation against the MI355X peak): algorithmic float32
    # FLOPs of model.py:51-64 on both padded images (296 kFLOP per pixel and image) over the stage's time,
    # against the dense f16 matrix peak - and what the kernels ISSUE: every multiply of layers 2..5 as three f16 products
    if "features" in stages and not lib_features:
        px = 2.0 * H * W
        algo_flop = px * (2 * 9 * 64 + 4 * 2 * 9 * 64 * 64)
        issued = px * 3 * 4 * 2 * 9 * 64 * 64
        t = stages["features"] * 1e-3
        rooflines["features"] = {"bound": "mfma", "achieved": round(algo_flop / t / 1e12, 1), "peak": MFMA_F16_PEAK_TFLOPS,
                                 "unit": "TFLOP/s", "frac": round(algo_flop / t / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                                 "issued_f16_tflops": round(issued / t / 1e12, 1),
                                 "issued_frac_of_peak": round(issued / t / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                                 "traffic": None, "launches_per_step": 1, "avg_launch_ms": round(stages["features"], 4),
                                 "algorithmic_flops_per_launch": int(algo_flop),
                                 "note": "whole conv stack of one pair (conv1 on the vector units + four matrix-core "
                                         "layers + normalisation); `achieved` counts the network's float32 FLOPs, "
                                         "`issued_f16_tflops` the three f16 products per multiply the split operands cost"}
    if "cost_volume" in stages and not args.exact:
        t = stages["cost_volume"] * 1e-3
        flop = 2.0 * 64 * voxels
        rooflines["cost_volume"] = {"bound": "hbm", "achieved": round(2 * vol_bytes / t / 1e9, 1), "peak": HBM_PEAK_GBS,
                                    "unit": "GB/s", "frac": round(2 * vol_bytes / t / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                                    "launches_per_step": counts["cost_volume"], "avg_launch_ms": round(stages["cost_volume"], 4),
                                    "algorithmic_bytes_per_launch": int(2 * vol_bytes),
                                    "mfma_issued_f16_tflops": round(3 * flop / t / 1e12, 2),
                                    "mfma_issued_frac_of_peak": round(3 * flop / t / 1e12 / MFMA_F16_PEAK_TFLOPS, 5),
                                    "note": "matching-cost GEMM: write-bound (16 FLOP per output byte), 3 f16 products per multiply"}
    elif "cost_volume" in stages:
        t = stages["cost_volume"] * 1e-3
        rooflines["cost_volume"] = {"bound": "hbm", "achieved": round(2 * vol_bytes / t / 1e9, 1), "peak": HBM_PEAK_GBS,
                                    "unit": "GB/s", "frac": round(2 * vol_bytes / t / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                                    "launches_per_step": counts["cost_volume"], "avg_launch_ms": round(stages["cost_volume"], 4),
                                    "algorithmic_bytes_per_launch": int(2 * vol_bytes),
                                    "note": "bit-exact float32 products in NumPy's pairwise order + border fill (the stage)"}
    dominant = max((k for k in rooflines if rooflines[k]["bound"] == "hbm" and k in algo), key=lambda k: per_step[k]) \
        if any(k in algo for k in rooflines) else None
    # SGM as a stage (what north_star's >= 50 % target is quoted on): 4 passes + the two layout changes
    sgm_kern_ms = (per_step.get("sgm_pass", 0.0) + per_step.get("sgm_pass_one_volume", 0.0) +
                   per_step.get("sgm_first_pass", 0.0))
    sgm_stage_ms = sgm_kern_ms + per_step.get("dhw_to_hwd", 0.0) + per_step.get("hwd_to_dhw", 0.0)
    sgm_span_ms = spans.get("sgm")     # the bracket around the four passes (free-running chains: one per chain, on its stream)
    if sgm_span_ms is not None and matcher.pixel_major():
        sgm_stage_ms = sgm_span_ms
    result.update({
        "roofline": dict(rooflines[dominant], kernel=dominant) if dominant else None,
        "rooflines": rooflines,
        # the two aggregations as stages (brackets around all their launches, both streams joined): what the chains of
        # concurrent one-volume launches achieve together
        "aggregation_stages": agg_stages,
        "sgm_stage": {"ms": round(sgm_stage_ms, 4), "algorithmic_bytes": int(4 * 2 * 2 * vol_bytes),
                      "how": ("bracket around the four passes of a chain, recorded on the chain's own stream (mean of the left "
                              "and the right chain, which run at the same time): both volumes' bytes over that span")
                      if sgm_span_ms is not None and matcher.pixel_major() else "sum of the launches' events",
                      "achieved_GBs": round(4 * 2 * 2 * vol_bytes / (sgm_stage_ms * 1e-3) / 1e9, 1) if sgm_stage_ms else None,
                      "frac_of_hbm_peak": round(4 * 2 * 2 * vol_bytes / (sgm_stage_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                      if sgm_stage_ms else None},
        # the SGM kernels alone: four directions, the first one carrying the DHW->HWD layout change; the separate
        # HWD->DHW launches excluded
        "sgm_kernels": {"ms": round(sgm_kern_ms, 4),
                        "frac_of_hbm_peak": round(4 * 2 * 2 * vol_bytes / (sgm_kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                        if sgm_kern_ms else None},
        "stage_ms_per_step": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
        # the same pair measured other ways (rank 0, 5 pairs each, outside `value`): launches issued one by one;
        # and match.py's own timed region, host images in / host map out over PCIe (pinned buffers)
        "ms_per_step_kernel_by_kernel": round(eager_ms, 3),
        "ms_per_step_host_in_host_out": round(host_io_ms, 3),
        "ms_per_step_library_features_kernel_by_kernel": round(lib_ms, 3) if lib_ms is not None else None,
        "sum_of_stage_ms": round(sum(per_step.values()), 3),
        # how much of the headline is a property of this image (10 / 3 graph replays each, same box, outside `value`)
        "unit_region_pixels": unit_fraction,
        "ms_per_step_without_skipping": round(noskip_ms, 3) if noskip_ms is not None else None,
        "ms_per_step_chains_joined_after_every_stage": round(joined_ms, 3) if joined_ms is not None else None,
        "natural_scene_ms_per_step": round(natural_ms, 3) if natural_ms is not None else None,
        "natural_scene": {"what": "synthetic.make_pair(kind='natural'): 1/f amplitude spectrum, 8 bit, standardised like "
                                  "match.py:120-121; the arm threshold is about one grey level, so almost every support "
                                  "region is the pixel itself (10 graph replays)",
                          "unit_region_pixels": natural_unit} if natural_ms is not None else None,
        # N pairs in flight on N streams (N matchers with their own workspaces and graphs): throughput, not latency
        "ms_per_pair_two_in_flight": in_flight.get(2), "ms_per_pair_four_in_flight": in_flight.get(4),
        "worst_case_ms_per_step": round(worst_ms, 3) if worst_ms is not None else None,
        "worst_case_scene": {"what": "synthetic.make_pair(texture=False): the flat blobs alone, support regions of several "
                                     "hundred pixels almost everywhere - the aggregation is bound by the reference's "
                                     "running sums (pf:157-161), not by bytes",
                             "unit_region_pixels": worst_unit} if worst_ms is not None else None,
        "parity": parity,
        "parity_violations": violations,
        # the other variant on the same box and pair (10 graph replays, outside `value`)
        ("fast_variant_ms_per_step" if is_default else "exact_variant_ms_per_step"):
            round(other_ms, 3) if other_ms is not None else None,
        "fast_variant_parity": other_parity,
    })
    result.update(ranks)
    if not args.no_cpu_baseline and world == 1:
        cores = args.cpu_cores if args.cpu_cores > 0 else max(1, min(16, (os.cpu_count() or 2) // 2))
        if not os.path.isfile(wpath):      # random-init run: hand the workers the same weights through a file
            import tempfile
            wpath = os.path.join(tempfile.mkdtemp(), "weights.npz")
            np.savez(wpath, **{"conv%d/%s" % (k + 1, n): a for k, (w, b) in enumerate(layers)
                               for n, a in (("weights", w), ("biases", b))})
        result["cpu_baseline"] = cpu_baseline(H, W, D, args.cpu_sample, cores, wpath)
    else:
        result["cpu_baseline"] = None
    print(json.dumps(result))
    mgpu.finalize()
    if violations:
        sys.stderr.write("bench: parity violated: %s\n" % "; ".join(violations))
        sys.exit(3)


if __name__ == "__main__":
    main()
