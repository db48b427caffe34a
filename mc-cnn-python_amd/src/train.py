"""Training of the matching network - drop-in for /root/reference/src/train.py (same command line), on PyTorch-ROCm.

    python train.py --list_dir LISTS --tensorboard_dir LOG --checkpoint_dir CKPT [-bs 128 -mr 0.2 -lr 0.002 -bt 0.9 ...]

What the reference's graph does (train.py:71-106) and what happens here:
  * three weight-shared towers (left, right+, right-) of model.NET on 11x11 patches (:76-78)   -> ONE NET applied to
    the three batches stacked into one [3B,11,11,1] batch (the towers ARE the same variables, AUTO_REUSE);
  * similarity = dot product of the L2-normalised 64-vectors (:85-87); loss = mean(max(0, margin - s+ + s-)) (:90-93);
  * tf.train.MomentumOptimizer(lr, beta) (:105-106): accum = beta*accum + grad; var -= lr*accum
    -> torch.optim.SGD(momentum=beta, dampening=0, nesterov=False), the same recurrence;
  * one mini-batch per training image per epoch, drawn by datagenerator.ImageDataGenerator (:159-164);
  * validation loss over val.txt every --val_freq epochs (:182-197); a checkpoint every --save_freq epochs (:176-180).
Checkpoints are `.npz` files (conv<k>/weights HWIO, conv<k>/biases, plus the momentum slots) named
`model_epoch<N>.ckpt.npz`; match.py's --resume and NET.restore read them (and the reference's TensorFlow bundles).
Differences from the reference a maintainer should know: checkpoints are written as `.npz` only (match.py / train.py of
THIS package read them and the reference's TensorFlow bundles, incl. the Momentum slots on --resume; the reference
cannot read the .npz - one-way compatibility); the logged hinge_loss is the loss of the batch BEFORE its update (the
reference re-evaluates the graph after the step, train.py:169-173); the patch sampler's RNG state is not checkpointed.
TensorBoard is not in this image: the two scalars the reference logs (hinge_loss, val_hinge_loss) go to
`<tensorboard_dir>/scalars.jsonl`, one JSON object per point with the reference's step numbering.
Multi-GPU (not in the reference): under torchrun every rank draws its own batches and the gradients are averaged with
all_reduce (RCCL) before the step - synchronous data parallelism; rank 0 writes logs and checkpoints.
Training the paper's way (not in the reference; off unless asked for): --sampler device keeps the images on the GPU and
cuts every batch there (datagenerator.DevicePatchSampler, csrc/sample.hip); with it --sampling pool shuffles every valid
ground-truth pixel of train.txt into one pool (an epoch is n_valid // batch_size steps instead of one per image),
--augment middlebury|kitti applies the paper's data set augmentation (every key has an --aug_<key> override),
--subpixel_centres keeps the fractional disparity; --lr_drop_epoch E --lr_drop_factor F divides the learning rate by F
from epoch E on (the paper: one tenfold drop).  Validation keeps pair sampling on val.txt, without augmentation.
Validation by error rate (the paper's model selection; not in the reference): --val_error matches every pair of val.txt
with the current weights (stereo_device.StereoMatcher, default hyper-parameters, ndisp from the calib.txt beside im0.png)
and scores the maps against disp0GT.pfm / mask0nocc.png on the device (evaluation.py), every --val_error_freq epochs on
rank 0; the pooled val_bad1.0_nonocc, val_bad2.0_nonocc, val_bad2.0_all and val_avgerr_all go to scalars.jsonl, and
--save_best keeps the checkpoint with the lowest val_bad2.0_nonocc as model_best.ckpt.npz.  Needs a GPU.
Other data sets (not in the reference): --dataset kitti2012|kitti2015 maps a listed left image to its right view and its
ground truth as the development kits lay them out (src/datasets.py) and reads the 16-bit disp_noc plane as float32 with
+inf where it holds no value, so every sampler works on the sparse truth as it does on Middlebury's.  --val_error then
matches with --ndisp, scores with mccnn_evaluate_kitti and logs val_d1_all, val_d1_nonocc (off by more than 3 px and 5 %
of the true disparity) and val_avgerr_all; --save_best keeps the lowest val_d1_all.
"""
import argparse
import json
import os
from datetime import datetime

import numpy as np

import datasets
import util
from datagenerator import AUGMENT_KEYS      # NumPy only: torch is imported in main(), after the GPU is pinned

parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                 description="training of the MC-CNN matching network (fast architecture)")
parser.add_argument("-g", "--gpu", type=str, default="0", action=util.ExplicitStore,
                    help="index of the GPU to train on (when not given, a HIP_VISIBLE_DEVICES already in the environment "
                         "stands; ignored under torchrun)")
parser.add_argument("-ps", "--patch_size", type=int, default=11, help="side of the square training patches")
parser.add_argument("-bs", "--batch_size", type=int, default=128, help="patch triplets per mini-batch")
parser.add_argument("-mr", "--margin", type=float, default=0.2, help="margin of the hinge loss")
parser.add_argument("-lr", "--learning_rate", type=float, default=0.002, help="step size")
parser.add_argument("-bt", "--beta", type=float, default=0.9, help="momentum (declared int in the reference, which "
                    "only works at its default 0.9)")
parser.add_argument("--list_dir", type=str, required=True, help="directory holding train.txt and val.txt (left-image lists)")
parser.add_argument("--tensorboard_dir", type=str, required=True, help="directory for the scalar log")
parser.add_argument("--checkpoint_dir", type=str, required=True, help="directory for the checkpoints")
parser.add_argument("--resume", type=str, default=None, help="checkpoint to start from (.npz of this script, or a "
                    "TensorFlow bundle prefix of the reference); default: fresh glorot-uniform weights")
parser.add_argument("--start_epoch", type=int, default=0, help="first epoch (inclusive)")
parser.add_argument("--end_epoch", type=int, default=14, help="last epoch (exclusive)")
parser.add_argument("--print_freq", type=int, default=10, help="log the training loss every this many batches")
parser.add_argument("--save_freq", type=int, default=1, help="write a checkpoint every this many epochs")
parser.add_argument("--val_freq", type=int, default=1, help="validate every this many epochs")
parser.add_argument("--seed", type=int, default=0, help="seed of the weight initialisation and the patch sampler")
parser.add_argument("--arch", choices=("fast", "accurate"), default="fast",
                    help="'fast': the reference's network and hinge loss; 'accurate': the paper's other network (112-map "
                         "tower, fully-connected decision network, sigmoid) trained with binary cross-entropy on the same "
                         "triplets - (left, right+) -> 1, (left, right-) -> 0; scalars bce_loss / val_bce_loss")
parser.add_argument("--num_fc_layers", type=int, default=3,
                    help="with --arch accurate: hidden fully-connected layers (Middlebury 3, KITTI 4)")
parser.add_argument("--sampler", choices=("host", "device"), default="host",
                    help="'host': the reference's sampler, patches cut with NumPy and copied to the GPU; 'device': the "
                         "images live on the GPU and one HIP launch cuts each batch (needs a GPU)")
parser.add_argument("--sampling", choices=("pair", "pool"), default="pair",
                    help="'pair': one mini-batch per training image per epoch (the reference); 'pool': mini-batches from "
                         "one shuffled pool of every valid pixel of the training set (the paper; needs --sampler device)")
parser.add_argument("--augment", choices=("none", "middlebury", "kitti"), default="none",
                    help="the paper's data set augmentation with the preset of that data set (needs --sampler device)")
for _key in AUGMENT_KEYS:
    parser.add_argument("--aug_" + _key, type=float, default=None,
                        help="overrides '%s' of the --augment preset (needs --sampler device)" % _key)
parser.add_argument("--subpixel_centres", action="store_true",
                    help="keep the fractional ground-truth disparity and the fractional displaced columns instead of the "
                         "reference's int() (the paper's rule; needs --sampler device)")
parser.add_argument("--lr_drop_epoch", type=int, default=None,
                    help="from this epoch on the learning rate is learning_rate / lr_drop_factor (default: never)")
parser.add_argument("--lr_drop_factor", type=float, default=10.0, help="see --lr_drop_epoch")
parser.add_argument("--val_error", action="store_true",
                    help="validate by the error rate of the whole pipeline: match every pair of val.txt with the current "
                         "weights and score it against its ground truth on the device (needs a GPU; rank 0)")
parser.add_argument("--val_error_freq", type=int, default=1, help="with --val_error: every this many epochs")
parser.add_argument("--save_best", action="store_true",
                    help="with --val_error: copy the checkpoint with the lowest val_bad2.0_nonocc (a KITTI --dataset: "
                         "val_d1_all) to model_best.ckpt.npz")
parser.add_argument("--dataset", choices=datasets.NAMES, default="middlebury",
                    help="the layout of the trees train.txt and val.txt name (src/datasets.py): where the right view and "
                         "the ground truth of a left image are, and how the ground truth is read.  A KITTI layout trains "
                         "on disp_noc (16-bit PNG, 0 = unknown) and --val_error then scores with the development kit's "
                         "rule: val_d1_all, val_d1_nonocc (off by more than 3 px and 5 %%), val_avgerr_all")
parser.add_argument("--ndisp", type=int, default=None,
                    help="with a KITTI --dataset and --val_error: the number of disparities searched (default %d, the "
                         "paper's)" % datasets.KITTI_NDISP)


def parse_args(argv=None):
    """parser.parse_args plus the rules between the flags: what only the device sampler can do asks for it by name."""
    args = parser.parse_args(argv)
    overrides = {k: getattr(args, "aug_" + k) for k in AUGMENT_KEYS if getattr(args, "aug_" + k) is not None}
    if args.sampler != "device":
        for given, flag in ((args.sampling == "pool", "--sampling pool"), (args.augment != "none", "--augment"),
                            (args.subpixel_centres, "--subpixel_centres")) + \
                tuple((True, "--aug_" + k) for k in overrides):
            if given:
                parser.error("%s requires --sampler device" % flag)
    if args.lr_drop_factor <= 0:
        parser.error("--lr_drop_factor must be positive")
    if args.save_best and not args.val_error:
        parser.error("--save_best requires --val_error")
    if args.val_error_freq < 1:
        parser.error("--val_error_freq must be positive")
    args.ndisp = datasets.resolve_ndisp(datasets.get(args.dataset), args.ndisp, parser.error)
    args.augment_overrides = overrides
    return args


def hinge_loss(features, batch_size, margin):
    """features: [3B,1,1,64] unit vectors of the stacked (left, right+, right-) batch -> mean hinge loss (train.py:80-93)."""
    f = features.reshape(3, batch_size, -1)
    cosine_pos = (f[0] * f[1]).sum(dim=-1)
    cosine_neg = (f[0] * f[2]).sum(dim=-1)
    return (margin - cosine_pos + cosine_neg).clamp(min=0.0).mean()


def bce_loss(logits_pos, logits_neg):
    """Binary cross-entropy of the accurate network (paper sec. 3.2): the mean of -log s over the (left, right+) pairs
    and -log(1 - s) over the (left, right-) pairs, s = sigmoid(logit), evaluated on the logits."""
    import torch
    import torch.nn.functional as F
    logits = torch.cat((logits_pos, logits_neg))
    target = torch.cat((torch.ones_like(logits_pos), torch.zeros_like(logits_neg)))
    return F.binary_cross_entropy_with_logits(logits, target)


class Trainer(object):
    """The trainable twin of model.NET: the same conv{k}/weights + biases as torch Parameters, forward through
    NET's own evaluation code, momentum SGD, (optional) gradient averaging across ranks."""

    def __init__(self, net, learning_rate, beta, margin):
        import torch
        self.net = net
        self.params = []
        for k in range(net.num_conv_layers):
            net.weights[k] = torch.nn.Parameter(net.weights[k].clone())
            net.biases[k] = torch.nn.Parameter(net.biases[k].clone())
            self.params += [net.weights[k], net.biases[k]]
        self.accurate = hasattr(net, "fc_weights")     # model.ACCURATE_NET: BCE on the decision network's logits
        if self.accurate:
            for k in range(len(net.fc_weights)):
                net.fc_weights[k] = torch.nn.Parameter(net.fc_weights[k].clone())
                net.fc_biases[k] = torch.nn.Parameter(net.fc_biases[k].clone())
                self.params += [net.fc_weights[k], net.fc_biases[k]]
        self.opt = torch.optim.SGD(self.params, lr=learning_rate, momentum=beta, dampening=0.0, nesterov=False)
        self.margin = margin

    def _stacked(self, batch_left, batch_right_pos, batch_right_neg):
        import torch
        x = torch.from_numpy(np.concatenate([batch_left, batch_right_pos, batch_right_neg], axis=0)).to(self.net.device)
        return x, batch_left.shape[0]

    def loss_stacked(self, x, B):
        """x: [3B,ps,ps,1] tensor on the network's device, the (left, right+, right-) batches stacked in that order
        (what DevicePatchSampler.next_batch returns)."""
        if self.accurate:
            f = self.net(x).reshape(3, B, -1)        # the three weight-shared towers as one batch
            return bce_loss(self.net.decision_logits(f[0], f[1]), self.net.decision_logits(f[0], f[2]))
        return hinge_loss(self.net(x), B, self.margin)

    def loss(self, batch_left, batch_right_pos, batch_right_neg):
        return self.loss_stacked(*self._stacked(batch_left, batch_right_pos, batch_right_neg))

    def step(self, batch_left, batch_right_pos, batch_right_neg):
        return self.step_stacked(*self._stacked(batch_left, batch_right_pos, batch_right_neg))

    def step_stacked(self, x, B):
        import torch.distributed as dist
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss_stacked(x, B)
        loss.backward()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            for p in self.params:            # synchronous data parallelism: average the gradients, then the same step
                dist.all_reduce(p.grad)
                p.grad /= dist.get_world_size()
        self.opt.step()
        return float(loss.detach())

    def state(self):
        """{name: array}: variables in TensorFlow's naming/layout plus the optimizer's momentum slots."""
        out = {}
        for k, (w, b) in enumerate(self.net.get_layers(), start=1):
            out["conv%d/weights" % k] = w
            out["conv%d/biases" % k] = b
        for k in range(self.net.num_conv_layers):
            for name, p in (("weights", self.net.weights[k]), ("biases", self.net.biases[k])):
                buf = self.opt.state.get(p, {}).get("momentum_buffer")
                if buf is not None:
                    a = buf.detach().cpu().numpy()
                    out["conv%d/%s/Momentum" % (k + 1, name)] = np.transpose(a, (2, 3, 1, 0)) if a.ndim == 4 else a
        if self.accurate:
            for k, (w, b) in enumerate(self.net.get_fc_layers(), start=1):
                out["fc%d/weights" % k] = w
                out["fc%d/biases" % k] = b
            for k in range(len(self.net.fc_weights)):
                for name, p in (("weights", self.net.fc_weights[k]), ("biases", self.net.fc_biases[k])):
                    buf = self.opt.state.get(p, {}).get("momentum_buffer")
                    if buf is not None:
                        a = buf.detach().cpu().numpy()
                        out["fc%d/%s/Momentum" % (k + 1, name)] = a.T if a.ndim == 2 else a
        return out

    def load_state(self, path):
        """Weights from an .npz of this script or a TensorFlow bundle; momentum slots when the .npz has them."""
        import torch
        import tf_checkpoint
        layers = tf_checkpoint.load_fast_net_weights(path)
        with torch.no_grad():
            for k, (w, b) in enumerate(layers):
                self.net.weights[k].copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(w, (3, 2, 0, 1)))))
                self.net.biases[k].copy_(torch.from_numpy(np.ascontiguousarray(b)))
        # the optimizer's momentum slots, as saver.restore brings them back in the reference (train.py:141-143):
        # from this script's .npz, or from the "<var>/Momentum" tensors of a TensorFlow bundle
        if os.path.isfile(path) and path.endswith(".npz"):
            z = np.load(path)
            slots = {k: z[k] for k in z.files if k.endswith("/Momentum")}
        else:
            slots = {k: v for k, v in tf_checkpoint.load_checkpoint(path, skip_slots=False).items()
                     if k.endswith("/Momentum")}
        for k in range(self.net.num_conv_layers):
            for name, p in (("weights", self.net.weights[k]), ("biases", self.net.biases[k])):
                a = slots.get("conv%d/%s/Momentum" % (k + 1, name))
                if a is not None:
                    a = np.transpose(a, (3, 2, 0, 1)) if a.ndim == 4 else a
                    self.opt.state[p]["momentum_buffer"] = torch.from_numpy(np.ascontiguousarray(a)).to(p.device)
        if self.accurate:
            _conv, fc = tf_checkpoint.load_accurate_net_weights(path)
            with torch.no_grad():
                for k, (w, b) in enumerate(fc):
                    self.net.fc_weights[k].copy_(torch.from_numpy(np.ascontiguousarray(w.T)))
                    self.net.fc_biases[k].copy_(torch.from_numpy(np.ascontiguousarray(b)))
            for k in range(len(self.net.fc_weights)):
                for name, p in (("weights", self.net.fc_weights[k]), ("biases", self.net.fc_biases[k])):
                    a = slots.get("fc%d/%s/Momentum" % (k + 1, name))
                    if a is not None:
                        a = a.T if a.ndim == 2 else a
                        self.opt.state[p]["momentum_buffer"] = torch.from_numpy(np.ascontiguousarray(a)).to(p.device)


VAL_ERROR_TAGS = ("val_bad1.0_nonocc", "val_bad2.0_nonocc", "val_bad2.0_all", "val_avgerr_all")
KITTI_VAL_ERROR_TAGS = ("val_d1_all", "val_d1_nonocc", "val_avgerr_all")     # D1 = (3 px, 5 %), whichever KITTI year


class PipelineValidator(object):
    """--val_error: the pairs of a list matched with `net` as it stands and scored on the device.  One StereoMatcher
    serves every epoch: it reads the net's own tensors, and the nets' packed-weight caches are keyed by the tensors'
    _version, which every optimiser step advances."""

    def __init__(self, net, list_file, layout=None, ndisp=None):
        import evaluation
        import stereo_device as sd
        self.ev = evaluation
        self.layout = layout if layout is not None else datasets.get("middlebury")
        self.ndisp = ndisp
        self.tags = KITTI_VAL_ERROR_TAGS if self.layout.kitti else VAL_ERROR_TAGS
        self.best_tag = self.tags[0] if self.layout.kitti else "val_bad2.0_nonocc"
        self.matcher = sd.StereoMatcher(net)
        with open(list_file, "r") as f:
            self.left_paths = [line.strip() for line in f if line.strip()]

    def run(self):
        """-> {tag: pooled value or None} over the pairs that have ground truth."""
        import torch
        ev, layout = self.ev, self.layout
        d1 = ((3.0, 0.05),)
        evaluator = layout.evaluator(d1 if layout.kitti else ev.DEFAULT_THRESHOLDS, device=self.matcher.device)
        with torch.no_grad():
            for left_path in self.left_paths:
                truth = layout.load_truth(left_path)
                if truth is None:
                    continue
                height, width, ndisp = layout.shape(left_path, self.ndisp)
                ev.check_shape(truth[0], (height, width), left_path)
                views = []
                for path in (left_path, layout.right(left_path)):       # as match.py standardises
                    g = util.read_gray(path).astype(np.float32)
                    views.append(torch.from_numpy((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1))).cuda())
                disparity = self.matcher.match(views[0], views[1], ndisp)
                evaluator.pair(disparity, torch.from_numpy(truth[0]).cuda(),
                               torch.from_numpy(truth[1]).cuda() if truth[1] is not None else None)
        pooled = evaluator.report()
        if layout.kitti:
            return {"val_d1_all": pooled.bad(3.0, "all"), "val_d1_nonocc": pooled.bad(3.0, "nonocc"),
                    "val_avgerr_all": pooled.figures["all"]["avgerr"]}
        return {"val_bad1.0_nonocc": pooled.bad(1.0, "nonocc"), "val_bad2.0_nonocc": pooled.bad(2.0, "nonocc"),
                "val_bad2.0_all": pooled.bad(2.0, "all"), "val_avgerr_all": pooled.figures["all"]["avgerr"]}


def main(argv=None):
    args = parse_args(argv)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    util.pin_gpu(args, world)     # an explicit -g pins the card (train.py:57), before torch initialises HIP

    import torch
    import distributed as mgpu
    import datagenerator
    from datagenerator import ImageDataGenerator
    from model import ACCURATE_NET, NET

    on_gpu = torch.cuda.is_available()
    if args.val_error and not on_gpu:
        parser.error("--val_error matches and scores the validation pairs on the GPU and no HIP device is visible "
                     "(there is no CPU fallback)")
    if on_gpu:
        torch.cuda.set_device(local_rank if world > 1 else 0)
    device = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    mgpu.init("nccl" if on_gpu else "gloo", device if on_gpu else None)

    os.makedirs(args.tensorboard_dir, exist_ok=True)
    os.makedirs(args.checkpoint_dir, exist_ok=True)
    ps = (args.patch_size, args.patch_size)
    # None keeps the generators on the reference's suffix replacement; a KITTI layout maps the paths and reads the truth
    layout = datasets.get(args.dataset) if args.dataset != "middlebury" else None
    if args.sampler == "device":
        import _hipabi
        _hipabi.require_device()                  # the cut is a HIP kernel; there is no CPU fallback
        augment = None
        if args.augment != "none" or args.augment_overrides:
            augment = dict({"none": datagenerator.AUGMENT_NONE, "middlebury": datagenerator.AUGMENT_MIDDLEBURY,
                            "kitti": datagenerator.AUGMENT_KITTI}[args.augment], **args.augment_overrides)
        train_generator = datagenerator.DevicePatchSampler(
            os.path.join(args.list_dir, "train.txt"), shuffle=True, patch_size=ps,
            rng=np.random.default_rng(args.seed + 1000 * rank), device=device, sampling=args.sampling,
            truncate=not args.subpixel_centres, augment=augment, batch_size=args.batch_size, world_size=world,
            layout=layout)
        val_generator = datagenerator.DevicePatchSampler(
            os.path.join(args.list_dir, "val.txt"), shuffle=False, patch_size=ps,
            rng=np.random.default_rng(args.seed + 7), device=device, layout=layout)
        train_batches_per_epoch = train_generator.steps_per_epoch
        train_step = lambda: trainer.step_stacked(train_generator.next_batch(args.batch_size), args.batch_size)
        val_loss = lambda: trainer.loss_stacked(val_generator.next_batch(args.batch_size), args.batch_size)
    else:
        train_generator = ImageDataGenerator(os.path.join(args.list_dir, "train.txt"), shuffle=True, patch_size=ps,
                                             rng=np.random.default_rng(args.seed + 1000 * rank), layout=layout)
        val_generator = ImageDataGenerator(os.path.join(args.list_dir, "val.txt"), shuffle=False, patch_size=ps,
                                           rng=np.random.default_rng(args.seed + 7), layout=layout)
        train_batches_per_epoch = train_generator.data_size
        train_step = lambda: trainer.step(*train_generator.next_batch(args.batch_size))
        val_loss = lambda: trainer.loss(*val_generator.next_batch(args.batch_size))
    val_batches_per_epoch = val_generator.data_size

    if args.arch == "accurate":
        net = ACCURATE_NET(None, input_patch_size=args.patch_size, num_conv_layers=(args.patch_size - 1) // 2,
                           batch_size=args.batch_size, device=device, seed=args.seed, num_fc_layers=args.num_fc_layers)
    else:
        net = NET(None, input_patch_size=args.patch_size, num_conv_layers=(args.patch_size - 1) // 2,
                  batch_size=args.batch_size, device=device, seed=args.seed)
    loss_tag = "bce_loss" if args.arch == "accurate" else "hinge_loss"
    trainer = Trainer(net, args.learning_rate, args.beta, args.margin)
    if args.resume is not None:
        trainer.load_state(args.resume)
    log = open(os.path.join(args.tensorboard_dir, "scalars.jsonl"), "a") if rank == 0 else None
    validator = PipelineValidator(net, os.path.join(args.list_dir, "val.txt"), layout,
                                  args.ndisp) if args.val_error and rank == 0 else None
    best = None          # the lowest val_bad2.0_nonocc (a KITTI layout: val_d1_all) so far

    def scalar(tag, value, step):
        if log is not None:
            log.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
            log.flush()

    if args.sampling == "pool":
        print("[{}] {}: {} training pairs, {} steps per epoch from a pool of {} pixels, {} validation pairs, {} rank(s) "
              "on {}".format(rank, datetime.now(), train_generator.data_size, train_batches_per_epoch,
                             train_generator.n_valid, val_batches_per_epoch, world, device))
    else:
        print("[{}] {}: {} training pairs, {} validation pairs, {} rank(s) on {}".format(
            rank, datetime.now(), train_batches_per_epoch, val_batches_per_epoch, world, device))
    for epoch in range(args.start_epoch, args.end_epoch):
        if args.lr_drop_epoch is not None:
            for group in trainer.opt.param_groups:
                group["lr"] = args.learning_rate / (args.lr_drop_factor if epoch >= args.lr_drop_epoch else 1.0)
        for batch in range(train_batches_per_epoch):
            loss = train_step()
            if (batch + 1) % args.print_freq == 0:
                scalar(loss_tag, loss, epoch * train_batches_per_epoch + batch)        # train.py:169-173
        if (epoch + 1) % args.save_freq == 0 and rank == 0:
            name = os.path.join(args.checkpoint_dir, "model_epoch" + str(epoch + 1) + ".ckpt.npz")
            np.savez(name, **trainer.state())
            print("[{}] {}: epoch {} saved to {}".format(rank, datetime.now(), epoch + 1, name))
        if validator is not None and (epoch + 1) % args.val_error_freq == 0:
            errors = validator.run()
            print("[{}] {}: epoch {} validation error: {}".format(rank, datetime.now(), epoch + 1, errors))
            for tag in validator.tags:
                if errors[tag] is not None:
                    scalar(tag, errors[tag], train_batches_per_epoch * (epoch + 1))
            key = errors[validator.best_tag]
            if args.save_best and key is not None and (best is None or key < best):
                best = key
                name = os.path.join(args.checkpoint_dir, "model_best.ckpt.npz")
                np.savez(name, **trainer.state())
                print("[{}] {}: epoch {} is the best so far ({} {}), saved to {}".format(
                    rank, datetime.now(), epoch + 1, validator.best_tag, key, name))
        if (epoch + 1) % args.val_freq == 0:
            with torch.no_grad():
                val_ls = sum(float(val_loss())
                             for _ in range(val_batches_per_epoch)) / (1. * max(val_batches_per_epoch, 1))
            print("[{}] {}: epoch {} validation loss: {}".format(rank, datetime.now(), epoch + 1, val_ls))
            scalar("val_" + loss_tag, val_ls, train_batches_per_epoch * (epoch + 1))        # train.py:196-197
        val_generator.reset_pointer()
        train_generator.reset_pointer()
    if log is not None:
        log.close()
    mgpu.finalize()


if __name__ == "__main__":
    main()
