"""Training steps per second with the host patch sampler and with the device patch sampler, on a seeded synthetic list of
15 pairs of 750 x 500 held in memory, mini-batches of 128 triplets, both architectures: `Trainer` fed by
ImageDataGenerator (patches cut with NumPy, copied to the GPU), by DevicePatchSampler in pair mode (the same batches,
cut on the GPU), in pool mode, and in pool mode with AUGMENT_MIDDLEBURY - and each sampler alone, without the network's
step.  The variants alternate in ONE process after a warm-up, three passes each.  Prints one JSON object (kept as
profiles/train_sampler.json).

    python tools/bench_train.py [--pairs 15 --height 500 --width 750 --batch_size 128 --steps 30 --passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mc-cnn-python_amd", "src"))

import numpy as np
import torch

import _hipabi as hip
import datagenerator as dg
import train
from model import ACCURATE_NET, NET


def synthetic_list(n_pairs, H, W, seed):
    """Random-texture left views, right views shifted by a disparity that is constant per band of rows, ground truth
    with a band of unknown (inf) pixels: [(left_u8, right_u8, gt)]."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n_pairs):
        scene = rng.integers(0, 256, size=(H, W + 64)).astype(np.uint8)
        shift = np.repeat(rng.integers(2, 33, size=(H + 24) // 25), 25)[:H]
        cols = 32 + np.arange(W)[None, :]
        left = np.take_along_axis(scene, np.broadcast_to(cols, (H, W)), axis=1)
        right = np.take_along_axis(scene, cols + shift[:, None], axis=1)        # right[y, x - s] = left[y, x]
        gt = np.broadcast_to(shift[:, None].astype(np.float32), (H, W)).copy()
        gt[:, :3] = np.inf
        pairs.append((left, right, gt))
    return pairs


class _HostInMemory(dg.ImageDataGenerator):
    data = None

    def read_image_list(self, _image_list):
        self.left_paths = ["pair%d/im0.png" % i for i in range(len(self.data))]
        self.right_paths = self.gt_paths = self.left_paths
        self.data_size = len(self.data)

    def prefetch(self):
        self.left_images = [self._standardise(p[0]) for p in self.data]
        self.right_images = [self._standardise(p[1]) for p in self.data]
        self.gt_images = [p[2] for p in self.data]


class _DeviceInMemory(dg.DevicePatchSampler):
    data = None
    read_image_list = _HostInMemory.read_image_list
    _load_images = _HostInMemory.prefetch


def rate(fn, steps):
    """Steps per second of `steps` calls of fn, the device drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=[round(x, 2) for x in xs])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=750)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed pass of a variant")
    ap.add_argument("--passes", type=int, default=3, help="timed passes of each variant (at least 3)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON object to this file")
    args = ap.parse_args(argv)
    passes, B = max(3, args.passes), args.batch_size
    device = hip.require_device()
    torch.cuda.set_device(0)
    _HostInMemory.data = _DeviceInMemory.data = synthetic_list(args.pairs, args.height, args.width, seed=0)

    def sampler(kind):
        if kind == "host":
            return _HostInMemory(None, shuffle=True, rng=np.random.default_rng(1))
        kw = {"device_pair": dict(sampling="pair"), "device_pool": dict(sampling="pool"),
              "device_pool_augmented": dict(sampling="pool", augment=dg.AUGMENT_MIDDLEBURY, truncate=False)}[kind]
        return _DeviceInMemory(None, shuffle=True, rng=np.random.default_rng(1), device=device, batch_size=B, **kw)

    kinds = ("host", "device_pair", "device_pool", "device_pool_augmented")
    samplers = {k: sampler(k) for k in kinds}

    def batch(k):
        """The next batch of sampler k; an epoch that runs out starts the next one, as train.py does."""
        s = samplers[k]
        try:
            return s.next_batch(B)
        except IndexError:
            s.reset_pointer()
            return s.next_batch(B)

    def on_device(k):
        """The sampler alone, up to the tensor the network reads: the host sampler's batch is stacked and copied."""
        if k == "host":
            return torch.from_numpy(np.concatenate(batch(k), axis=0)).to(device)
        return batch(k)

    result = dict(shape=dict(pairs=args.pairs, height=args.height, width=args.width, batch_size=B, patch_size=11),
                  steps_per_pass=args.steps, passes=passes, n_valid=samplers["device_pool"].n_valid,
                  steps_per_epoch={k: (s.steps_per_epoch if k != "host" else s.data_size) for k, s in samplers.items()},
                  sampler_alone_steps_per_s={}, train_steps_per_s={})
    alone = {k: [] for k in kinds}
    for k in kinds:
        rate(lambda: on_device(k), 5)
    for _ in range(passes):                            # alternately, so that drift hits every variant alike
        for k in kinds:
            alone[k].append(rate(lambda: on_device(k), args.steps))
    result["sampler_alone_steps_per_s"] = {k: spread(v) for k, v in alone.items()}

    for arch in ("fast", "accurate"):
        trainers = {}
        for k in kinds:                                # every variant its own network: the same work per step
            net = (ACCURATE_NET if arch == "accurate" else NET)(None, batch_size=B, device=device, seed=0)
            trainers[k] = train.Trainer(net, 0.002, 0.9, 0.2)

        def step(k):
            if k == "host":
                return trainers[k].step(*batch(k))
            return trainers[k].step_stacked(batch(k), B)

        runs = {k: [] for k in kinds}
        for k in kinds:
            rate(lambda: step(k), 5)
        for _ in range(passes):
            for k in kinds:
                runs[k].append(rate(lambda: step(k), args.steps))
        result["train_steps_per_s"][arch] = {k: spread(v) for k, v in runs.items()}
        med = {k: statistics.median(v) for k, v in runs.items()}
        result.setdefault("device_pair_over_host", {})[arch] = med["device_pair"] / med["host"]
    text = json.dumps(result, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return result


if __name__ == "__main__":
    main()
