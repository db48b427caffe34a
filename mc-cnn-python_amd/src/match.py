"""Drop-in for /root/reference/src/match.py: same command line, same output files, MI355X hot path.

    python match.py -g 0 --list_file LIST --resume CKPT_PREFIX --data_dir DATA --save_dir OUT -t TAG -s 0 -e 14

For every left image `.../im0.png` in the list (index window [start, end] inclusive, match.py:83-91) it reads
im1.png + calib.txt beside it, standardises both views, runs the timed region (features -> cost volume -> CBCA x2
-> SGM -> CBCA x16 -> WTA -> interpolation -> sub-pixel -> median -> bilateral) on one GPU and writes
    <save_dir>/submit_<tag>/<rel>/disp0MCCNN.pfm, timeMCCNN.txt   and   <save_dir>/submit_<tag>_imgs/<rel>/disp0MCCNN.pgm
exactly where the reference does (match.py:99-110, 182-184).

By default every stage after the conv features is bit-identical to the reference's NumPy code on the same inputs.
Addition: --fast computes the cost volume on the matrix cores instead of in NumPy's summation order (<= 2e-6 per score;
near-ties in the WTA can then resolve differently) and leaves every other stage as it is - a few per cent faster;
--fast --separable_cbca adds the aggregation through float64 prefix sums on plane-major volumes (<= 1e-6 per
iteration), the fast variant of rounds 2-3, which the bit-exact aggregation has overtaken since.
--pipeline streams the list (list_matcher.py): decoder threads, grey conversion + standardisation on the device, one
hipGraph replay per pair where a shape repeats, a writer thread - the same files, byte for byte.
--confidence msm,mmn,cur,lrc (any subset) writes the confidence planes of every map, conf0MCCNN_<measure>.pfm beside
disp0MCCNN.pfm, in all three loops; with --evaluate their sparsification figures join evalMCCNN.json and eval.json.
--views both writes the post-processed RIGHT disparity map as well: disp1MCCNN.pfm / .pgm beside the left files (and
conf1MCCNN_<measure>.pfm with --confidence), in all three loops; with --evaluate it is scored against disp1GT.pfm (and
mask1nocc.png) and every evaluation file gains a "right" block.  Middlebury layout only.
--evaluate --eval_quantiles 50,90,95,99 adds the error quantiles (Middlebury's A50 ... A99) of every scored map, selected
exactly on the device, and the list's pooled quantiles at 16 bits, in all three loops.  Middlebury layout only.
--vertical_offset auto|N matches a pair whose right image sits N rows low along that offset; auto measures N per pair on
the device and writes verticalMCCNN.json beside disp0MCCNN.pfm, the same bytes in all three loops.
--vertical_offset grid measures one offset per cell of --vertical_offset_grid GHxGW cells instead (a rolled rig, unequal
focal lengths); verticalMCCNN.json then also carries grid, offsets, cell_totals and cell_shares.
--depth writes the left view's depth plane, depth0MCCNN.pfm, and --point_cloud [--max_depth Z] its ordered point cloud,
points0MCCNN.ply, beside disp0MCCNN.pfm from the pair's calib.txt (cam0, doffs, baseline; --calib overrides it), computed
on the device behind the map, the same bytes in all three loops.  Middlebury layout only.
Multi-GPU: launch one process per GPU with different -g / -s / -e, as the reference intends (match.py:17, 26-28),
or use `torchrun --nproc-per-node N match.py ...`: rank r then takes the pairs i = r (mod N) of the window.
"""
import argparse
import collections
import contextlib
import json
import os
import time
from datetime import datetime

import numpy as np

import datasets
import evaluation          # (neither module touches torch or the GPU on import: util.pin_gpu comes first, in main)
import list_matcher
import util
from calibration import Calibration, point_pixels, write_ply
from semi_dense_rule import SemiDenseRule

# Flag names, types and defaults are the reference's command line (match.py:15-43) - that is the drop-in contract;
# the help texts are this project's.
parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                 description="MC-CNN stereo matching of a list of Middlebury-style pairs on one MI355X")
parser.add_argument("-g", "--gpu", type=str, default="0", action=util.ExplicitStore,
                    help="index of the GPU this process uses (when not given, a HIP_VISIBLE_DEVICES already in the "
                         "environment stands; ignored under torchrun: one rank per GPU)")
parser.add_argument("-ps", "--patch_size", type=int, default=11,
                    help="receptive field of the matching network (11 = five 3x3 layers)")
parser.add_argument("--list_file", type=str, required=True, help="text file with one left-image path (.../im0.png) per line")
parser.add_argument("--resume", type=str, default=None,
                    help="network weights: TensorFlow checkpoint prefix as written by the reference's train.py, or an "
                         ".npz of conv<k>/weights and conv<k>/biases")
parser.add_argument("--data_dir", type=str, required=True, help="root of the input tree (prefix of the listed paths)")
parser.add_argument("--save_dir", type=str, required=True, help="root under which submit_<tag>/ and submit_<tag>_imgs/ are written")
parser.add_argument("-t", "--tag", type=str, required=True, help="name of this run (part of the output directory names)")
parser.add_argument("-s", "--start", type=int, required=True,
                    help="first list index to match (inclusive) - split a list over several processes with -s/-e")
parser.add_argument("-e", "--end", type=int, required=True, help="last list index to match (inclusive)")

# hyper-parameters, defaults from the MC-CNN paper as in match.py:31-43 (the three CBCA values are declared float there
# but only work as the ints they default to - they are coerced with int() below)
parser.add_argument("--cbca_intensity", type=float, default=0.02, help="CBCA: largest |I(q) - I(p)| along a support arm")
parser.add_argument("--cbca_distance", type=float, default=14, help="CBCA: arm length limit (arms are shorter than this)")
parser.add_argument("--cbca_num_iterations1", type=float, default=2, help="CBCA iterations before SGM")
parser.add_argument("--cbca_num_iterations2", type=float, default=16, help="CBCA iterations after SGM")
parser.add_argument("--sgm_P1", type=float, default=2.3, help="SGM: penalty for a disparity change of one")
parser.add_argument("--sgm_P2", type=float, default=55.9, help="SGM: penalty for larger disparity changes")
parser.add_argument("--sgm_Q1", type=float, default=4, help="SGM: penalties divided by this where one view has an intensity edge")
parser.add_argument("--sgm_Q2", type=float, default=8, help="SGM: penalties divided by this where both views have one")
parser.add_argument("--sgm_D", type=float, default=0.08, help="SGM: intensity difference that counts as an edge")
parser.add_argument("--sgm_V", type=float, default=1.5, help="SGM: P1 is divided by this in the vertical directions")
parser.add_argument("--blur_sigma", type=float, default=6, help="bilateral filter: spatial sigma")
parser.add_argument("--blur_threshold", type=float, default=2, help="bilateral filter: intensity gate")
# additions of this implementation
parser.add_argument("--fast", action="store_true",
                    help="the cost volume on the matrix cores (split-f16 operands, <= 2e-6 per score) in front of the "
                         "bit-exact stages: a few per cent faster, final map within the stated tolerance "
                         "(src/tolerances.py).  Without it every stage after the conv features is bit-identical to the "
                         "reference's NumPy code")
parser.add_argument("--separable_cbca", action="store_true",
                    help="with --fast: also the separable float64-prefix aggregation on plane-major volumes (<= 1e-6 per "
                         "iteration; the fast variant of rounds 2-3, slower than the default since round 4)")
parser.add_argument("--exact", action="store_true", help="(default; kept for compatibility) the bit-exact variants")
parser.add_argument("--features", choices=("library", "split_f16"), default=None,
                    help="conv feature stack: 'split_f16' (default where the network is 3x3 / 64 maps: the hand-written "
                         "matrix-core kernels, float32 operands as two f16 parts, as close to a float64 evaluation as the "
                         "library) or 'library' (float32 convolutions of MIOpen, 1.5 ms slower per 750x500 pair).  A pair "
                         "whose activations leave the kernels' range is repeated with the library automatically")
parser.add_argument("--pairs_in_flight", type=int, default=1,
                    help="stereo pairs matched concurrently on this GPU, each on its own HIP stream with its own "
                         "workspace.  The kernels of a KITTI-sized or smaller pair do not fill 256 CUs (a 256x256x64 "
                         "pair reaches a third of the throughput of a 750x500x256 one); 2 overlaps the launch ramps of "
                         "one pair with the other.  Results are identical; timeMCCNN.txt then holds each pair's own "
                         "wall time, overlap included")
parser.add_argument("--pipeline", action="store_true",
                    help="stream the list (src/list_matcher.py): reader threads decode the PNGs to raw bytes in pinned "
                         "host memory ahead of the GPU, grey conversion and standardisation run on the device "
                         "(bit-identical to the host's), a shape that repeats is replayed as one hipGraph per pair, and a "
                         "writer thread writes the files.  Same files as without the flag, byte for byte; every other "
                         "flag keeps its meaning.  timeMCCNN.txt then holds, as with --pairs_in_flight, the pair's own "
                         "wall time from the enqueue of its host-to-device copy to its map being on the host, overlap "
                         "with other pairs (and a graph capture, where the pair paid one) included")
parser.add_argument("--readers", type=int, default=4, help="with --pipeline: decoder threads")
parser.add_argument("--arch", choices=("fast", "accurate"), default="fast",
                    help="network architecture: 'fast' (the reference's: dot product of normalised 64-vectors) or 'accurate' "
                         "(the paper's other network: 112-map tower + a fully-connected decision network evaluated for "
                         "every pixel and disparity on the matrix cores; --resume is then an .npz with fc<k>/ variables; "
                         "--fast selects its plain-f16 precision)")
parser.add_argument("--num_fc_layers", type=int, default=3,
                    help="with --arch accurate: hidden fully-connected layers (Middlebury 3, KITTI 4)")
parser.add_argument("--decision", choices=("auto", "kernel", "library"), default="auto",
                    help="with --arch accurate: the decision stage by the hand-written kernel, by float32 library "
                         "matmuls, or whichever serves the pair")
# opt-in departures from the reference's results: what the MC-CNN paper does and the reference names but leaves out
parser.add_argument("--paper_support_regions", action="store_true",
                    help="CBCA support regions intersected with the other view's at every disparity (paper sec. 4.1; "
                         "the reference skips this as impractical, process_functional.py:122-144)")
parser.add_argument("--paper_interpolation", action="store_true",
                    help="fill mismatches from 16 rays and occlusions from the left (paper sec. 4.4; "
                         "process_functional.py:318, :361 note the reference uses 4 directions and the right)")
parser.add_argument("--paper_sgm", action="store_true",
                    help="semiglobal matching as the paper defines it: the four directions each computed from the same "
                         "volume and averaged (the reference composes them one after the other on one array, "
                         "process_functional.py:195-210, and its average is the identity)")
parser.add_argument("--vertical_range", type=int, default=0,
                    help="for imperfectly rectified pairs: every pixel is also compared with the other view's pixels up to "
                         "this many rows above and below (0 .. 4) and keeps its best score per disparity "
                         "(include/mccnn.h: mccnn_cost_volume_vertical_hwd); everything behind the cost volume is "
                         "unchanged.  0 (default): the reference's row-to-row comparison.  Costs a point or two on "
                         "well-rectified pairs and 4 x range + 2 times the cost volume's products; bit-exact fast "
                         "network only: not with --fast, --separable_cbca, --paper_support_regions or --arch accurate")
parser.add_argument("--vertical_offset", type=str, default="0", metavar="auto|grid|N",
                    help="for pairs whose right image sits N rows low (N in -8 .. 8): the cost volume is taken against row "
                         "h + N of the other view (include/mccnn.h: mccnn_cost_volume_offset_hwd), --vertical_range "
                         "searched around it.  'auto': N is measured per pair on the device from the pair's features "
                         "(mccnn_vertical_profile) and written to verticalMCCNN.json beside the map (a KITTI --dataset: "
                         "submit_<tag>/vertical/NNNNNN_10.json).  'grid': one N per cell of --vertical_offset_grid, measured "
                         "the same way, for a residual that grows with the column or the row and averages to nothing "
                         "(mccnn_vertical_field_select, mccnn_cost_volume_field_hwd).  0 (default): nothing changes.  "
                         "Available where --vertical_range is")
parser.add_argument("--vertical_offset_grid", type=str, default="3x4", metavar="GHxGW",
                    help="--vertical_offset grid: the cells down and across (1 .. 8 each); clamped per pair to the image's "
                         "64-column blocks and to row bands of at least 8 measured rows, and written back as 'grid'")
parser.add_argument("--vertical_offset_max", type=int, default=4,
                    help="--vertical_offset auto: the largest offset that is measured, in rows either way (1 .. 8)")
parser.add_argument("--vertical_offset_rows", type=int, default=8,
                    help="--vertical_offset auto: every this many rows one row takes part in the measurement (>= 1)")
parser.add_argument("--numpy1_promotion", action="store_true",
                    help="evaluate the sub-pixel formula as NumPy < 2 promotes its scalars (float64, rounded once), "
                         "i.e. as the reference's own Python 2.7 environment does; differs by <= 2.5e-5 px")
parser.add_argument("--evaluate", action="store_true",
                    help="score every map against the disp0GT.pfm (and mask0nocc.png) beside its im0.png, on the device "
                         "(src/evaluation.py): bad-pixel rates, invalid pixels, average and RMS error over all pixels with "
                         "ground truth and over the non-occluded ones.  Writes evalMCCNN.json beside each disp0MCCNN.pfm and "
                         "submit_<tag>/eval.json (eval_rank<r>.json under torchrun) with the pooled totals; a pair without "
                         "ground truth is matched as usual and listed as skipped.  Every other output stays byte-identical")
parser.add_argument("--eval_thresholds", type=str, default=None,
                    help="with --evaluate: the bad-pixel thresholds in pixels, 1 to 8 comma-separated values (default: "
                         "0.5,1,2,4).  With a KITTI --dataset every item is abs[:rel] - a pixel is bad when its error "
                         "exceeds abs pixels and rel times the true disparity - and the default is the data set's own: "
                         "3:0.05 (D1) for kitti2015, 2,3,4,5 for kitti2012")
parser.add_argument("--eval_quantiles", type=str, default=None,
                    help="with --evaluate: the error quantiles of every map in per cent, 1 to 8 comma-separated values in "
                         "(0, 100] with at most four decimals, e.g. 50,90,95,99 for Middlebury's A50, A90, A95 and A99: the "
                         "exact nearest-rank quantiles of the error over the scored pixels of each region, selected on the "
                         "device (include/mccnn.h), \"quantiles\" in evalMCCNN.json and eval.json; the list's pooled "
                         "quantiles carry the top 16 bits of the exact ones.  Not with a KITTI --dataset.  Without it "
                         "every file keeps its bytes")
parser.add_argument("--dataset", choices=datasets.NAMES, default="middlebury",
                    help="the layout of the input tree and the format of the results (src/datasets.py).  'middlebury': "
                         "im0.png / im1.png / calib.txt per directory, PFM out.  'kitti2015': the list names "
                         ".../image_2/NNNNNN_10.png, the right view is under image_3, the ground truth under disp_occ_0 and "
                         "disp_noc_0 (16-bit PNG); the map is written as the development kit's 16-bit PNG to "
                         "submit_<tag>/disp_0/, the time to submit_<tag>/time/, the evaluation to submit_<tag>/eval/.  "
                         "'kitti2012': colored_0 / colored_1 or image_0 / image_1, disp_occ / disp_noc, maps in submit_<tag>/")
parser.add_argument("--ndisp", type=int, default=None,
                    help="with a KITTI --dataset: the number of disparities searched (default %d, the paper's; a "
                         "Middlebury pair's comes from its calib.txt)" % datasets.KITTI_NDISP)
parser.add_argument("--eval_interpolate", action="store_true",
                    help="with --evaluate and a KITTI --dataset: fill the pixels without a disparity from their "
                         "neighbours as the development kit does before scoring (on the device).  Without it they count "
                         "as bad, as they do for Middlebury")
parser.add_argument("--confidence", type=str, default=None,
                    help="confidence measures of every map, a comma-separated subset of msm,mmn,cur,lrc (negated winning "
                         "cost, margin to the runner-up, curvature at the winner, negated left-right difference; larger = "
                         "more confident; include/mccnn.h defines them): one more launch per pair, and one float32 PFM per "
                         "measure, conf0MCCNN_<measure>.pfm beside disp0MCCNN.pfm (a KITTI --dataset: "
                         "submit_<tag>/conf_<measure>/NNNNNN_10.pfm).  With --evaluate the measures are scored by the area "
                         "under their sparsification curves (\"sparsification\" in evalMCCNN.json and eval.json).  "
                         "Every other output stays byte-identical")
parser.add_argument("--eval_auc_threshold", type=str, default=None,
                    help="with --evaluate --confidence: the error that makes a pixel bad on the sparsification curve, in "
                         "pixels (default 1.0); with a KITTI --dataset abs[:rel] (default 3:0.05)")
parser.add_argument("--views", choices=("left", "both"), default="left",
                    help="'both': also the post-processed right disparity map (the left view's rules on the mirrored pair, "
                         "include/mccnn.h), written as disp1MCCNN.pfm / disp1MCCNN.pgm beside the left files, with "
                         "--confidence conf1MCCNN_<measure>.pfm; with --evaluate it is scored against disp1GT.pfm (and "
                         "mask1nocc.png) beside im0.png: a \"right\" block in evalMCCNN.json and eval.json, a pair without "
                         "disp1GT.pfm listed as skipped for the right view.  timeMCCNN.txt stays the whole pair's time.  "
                         "Not with a KITTI --dataset.  Without it every file keeps its bytes")
parser.add_argument("--semi_dense", type=str, default=None, metavar="RULE",
                    help="a semi-dense map beside every map: comma-separated items lr (keep left-right matches), "
                         "<msm|mmn|cur|lrc>:<min> (keep pixels whose confidence reaches min; the measure must be among "
                         "--confidence) and speckle:<min_size>[:<max_diff>] (drop 4-connected blobs of similar disparity "
                         "smaller than min_size; max_diff defaults to 1.0), e.g. lr,speckle:20:1 (include/mccnn.h defines "
                         "them).  Written as disp0MCCNN_s.pfm beside disp0MCCNN.pfm (--views both: also disp1MCCNN_s.pfm), "
                         "dropped pixels as inf; with --evaluate a \"semi_dense\" block (the sparse map's figures, its "
                         "density and the bad share among the kept pixels) in evalMCCNN.json and eval.json; "
                         "--eval_quantiles and the sparsification stay figures of the dense map.  Not with a KITTI "
                         "--dataset.  Without it every file keeps its bytes")
parser.add_argument("--depth", action="store_true",
                    help="the left view's depth plane beside every map, depth0MCCNN.pfm: Z = baseline * f / (d + doffs) of "
                         "the pair's calib.txt (cam0, doffs, baseline; Middlebury 2014's relation, Z in the unit of the "
                         "baseline, mm there), pixels without a depth as inf; one more launch per pair on the device "
                         "(include/mccnn.h: mccnn_depth).  Always of the dense map.  Not with a KITTI --dataset.  Without it "
                         "every file keeps its bytes")
parser.add_argument("--point_cloud", action="store_true",
                    help="the left view's point cloud beside every map, points0MCCNN.ply: binary little-endian PLY, x y z "
                         "float32 and the grey value of the left image as intensity uchar, one vertex per pixel with a "
                         "depth in raster order (include/mccnn.h: mccnn_reproject_points, an ordered compaction on the "
                         "device).  With --semi_dense the cloud is the sparse map's: dropped pixels are no points.  Not "
                         "with a KITTI --dataset.  Without it every file keeps its bytes")
parser.add_argument("--max_depth", type=float, default=None, metavar="Z",
                    help="with --point_cloud: only pixels with a depth of at most Z become points (default: every pixel with "
                         "a finite depth)")
parser.add_argument("--calib", type=str, default=None, metavar="fx,fy,cx,cy,baseline[,doffs]",
                    help="with --depth / --point_cloud: this calibration for every pair, instead of each pair's calib.txt")

CONFIDENCE_MEASURES = ("msm", "mmn", "cur", "lrc")      # stereo_device.CONFIDENCE_MEASURES (not imported before the GPU is pinned)


def parse_confidence(text):
    """'mmn,lrc' -> ('mmn', 'lrc') in plane order; () for None."""
    if text is None:
        return ()
    names = [t.strip() for t in str(text).split(",") if t.strip()]
    if not names or len(set(names)) != len(names) or any(n not in CONFIDENCE_MEASURES for n in names):
        raise ValueError("expected a comma-separated subset of %s without repeats, got %r" % (",".join(CONFIDENCE_MEASURES), text))
    return tuple(n for n in CONFIDENCE_MEASURES if n in names)


# different file names (the Middlebury layout's: src/datasets.py)
left_image_suffix = datasets.Middlebury.left_suffix
left_gt_suffix = datasets.Middlebury.gt_suffix
right_image_suffix = datasets.Middlebury.right_suffix
right_gt_suffix = datasets.Middlebury.right_gt_suffix
calib_suffix = datasets.Middlebury.calib_suffix

out_file = datasets.Middlebury.out_file
out_img_file = datasets.Middlebury.out_img_file
out_time_file = datasets.Middlebury.out_time_file
out_eval_file = datasets.Middlebury.out_eval_file


def parse_vertical_offset(text):
    """--vertical_offset: "auto", "grid", or an integer in [-8, 8]; None for anything else."""
    if text in ("auto", "grid"):
        return text
    try:
        value = int(text)
    except ValueError:
        return None
    return value if -8 <= value <= 8 else None


def parse_vertical_offset_grid(text):
    """--vertical_offset_grid: "GHxGW" with both in [1, 8] as (gh, gw); None for anything else."""
    try:
        grid = tuple(int(p) for p in text.lower().split("x"))
    except ValueError:
        return None
    return grid if len(grid) == 2 and all(1 <= g <= 8 for g in grid) else None


def hyper_parameters(args):
    return dict(cbca_intensity=args.cbca_intensity, cbca_distance=int(args.cbca_distance),
                cbca_num_iterations1=int(args.cbca_num_iterations1),
                cbca_num_iterations2=int(args.cbca_num_iterations2),
                sgm_P1=args.sgm_P1, sgm_P2=args.sgm_P2, sgm_Q1=args.sgm_Q1, sgm_Q2=args.sgm_Q2, sgm_D=args.sgm_D,
                sgm_V=args.sgm_V, blur_sigma=args.blur_sigma, blur_threshold=args.blur_threshold)


# a pair launched and not yet written: what crosses to the host for its map, its PairResult on the device with the map
# that is scored (layout.device_output states both), the event behind all of it, the start of its time, its paths, the
# matcher's inputs (a repeat needs them), its slot and its scoring record (evaluation.Scored, or None)
Pending = collections.namedtuple("Pending", "crossing result done started paths images slot scored")


class ListLoop(object):
    """The list loop without --pipeline: the host decodes and standardises a pair, launches it on its slot (one matcher
    and, with --pairs_in_flight N > 1, one stream per slot) and writes its files when the slot comes round again.

    layout: datasets.py; redo: stereo_device.SaturationRedo; scorer: evaluation.ListScorer or None (--evaluate);
    save(PairResult of host arrays, paths): the files of what crossed to the host; save_vertical(offset, totals, paths[,
    field, cell_totals]) (--vertical_offset auto | grid): the file of the pair's measured row offset, copied out behind
    the pair on its stream."""

    def __init__(self, layout, matchers, streams, redo, scorer, save, rank, save_vertical=None, calibration=None):
        import torch
        self.torch = torch
        self.layout, self.matchers, self.streams, self.redo, self.scorer = layout, matchers, streams, redo, scorer
        self.save, self.rank, self.save_vertical = save, rank, save_vertical
        self.calibration = calibration      # --depth / --point_cloud: paths -> the pair's Calibration, a launch argument
        self.pending = []            # oldest first

    def _stream(self, slot):
        return self.torch.cuda.stream(self.streams[slot]) if len(self.matchers) > 1 else contextlib.nullcontext()

    def _to_device(self, truth):
        """(ground truth, mask or None) of the host on the device, behind the pair on its stream."""
        if truth is None:
            return None
        return (self.torch.from_numpy(truth[0]).cuda(),
                self.torch.from_numpy(truth[1]).cuda() if truth[1] is not None else None)

    def _matched(self, matcher, images, scoring, paths):
        """One pair on `matcher`: ((what crosses to the host for its map, copies of its measured row offset and totals or
        None), its PairResult with the map that is scored) - the map, or a KITTI layout's 16-bit code and what it holds,
        behind the map on the current stream."""
        if self.calibration is not None:
            matcher.set_calibration(self.calibration(paths))
        result = matcher.result_of(matcher.match(*images))
        crossing, kept = self.layout.device_output(result.map, scoring)
        vertical = None
        if self.save_vertical is not None:       # (the slot's next pair overwrites the workspace's)
            vertical = tuple(b.clone() for b in matcher.vertical_buffers(images[0].shape[0], images[0].shape[1], images[2]))
        return (crossing, vertical), result._replace(map=kept)

    def launch(self, slot, index, paths, left_image, right_image, ndisp, truth, truth_right):
        """The timed region (match.py:129-179): host arrays in, host array out, device-synchronised - from here to
        finish().  With several pairs in flight the pair runs on its slot's stream."""
        torch = self.torch
        started = time.time()
        with self._stream(slot):
            images = (torch.from_numpy(left_image).cuda(), torch.from_numpy(right_image).cuda(), ndisp)
            crossing, result = self._matched(self.matchers[slot], images, truth is not None, paths)
            scored = None                    # the evaluation: behind the map and what is scored, on this stream
            if self.scorer is not None:
                scored = self.scorer.begin(index, paths["left"], self._to_device(truth), self._to_device(truth_right))
            if scored is not None:
                self.scorer.score(scored, result, slot)
            done = torch.cuda.Event()
            done.record()
        self.pending.append(Pending(crossing, result, done, started, paths, images, slot, scored))

    def finish(self):
        """Collects and writes the oldest pair."""
        p = self.pending.pop(0)
        p.done.synchronize()

        def rematch():
            library = self.redo.matcher()
            print("[{}] ".format(self.rank) + self.redo.notice(p.paths["out"]))
            return self._matched(library, p.images, p.scored is not None, p.paths)
        crossing, result = list_matcher.slot_comes_round(self.redo, rematch, self.scorer, p.scored, p.result, p.slot,
                                                         lambda: self._stream(p.slot),
                                                         self.torch.cuda.synchronize) or (p.crossing, p.result)
        # (the float32 map, or a KITTI layout's 16-bit plane)
        crossing, vertical = crossing
        host = result._replace(map=crossing).apply(lambda t: t.cpu().numpy())
        if vertical is not None:
            vertical = tuple(t.cpu().numpy() for t in vertical)
        seconds = time.time() - p.started
        self.save(host, p.paths)
        if vertical is not None:
            self.save_vertical(vertical[0], vertical[1], p.paths, *vertical[2:])
        util.saveTimeFile(seconds, p.paths["out_time"])
        print("[{}] {}: {:.3f} s -> {}".format(self.rank, datetime.now(), seconds, p.paths["out"]))
        if p.scored is not None:
            self.scorer.publish(p.scored, p.paths["out_eval"])

    def run(self, indices, paths, shape, footprint):
        """paths(index) -> the pair's inputs and outputs; shape(left path) -> (H, W, ndisp); footprint(H, W, ndisp) ->
        the workspace's bytes, and refuses a shape outside what the kernels serve (ValueError naming the limit; each
        matcher checks its own workspace against the free device memory before it allocates it)."""
        layout, in_flight = self.layout, len(self.matchers)
        last_shape = None
        for launched, index in enumerate(indices):
            p = paths(index)
            left_path, right_path = p["left"], p["right"]
            for d in p["dirs"]:
                util.recurMk(os.path.abspath(d))
            height, width, ndisp = shape(left_path)
            print("[{}] pair {}: {} | {}  ({}x{}, ndisp {})".format(self.rank, index, left_path, right_path, width, height, ndisp))
            nbytes = footprint(height, width, ndisp)
            if (height, width, ndisp) != last_shape:
                print("[{}] workspace {:.2f} GB ({} pair(s) in flight)".format(self.rank, nbytes / 1e9, in_flight))
                last_shape = (height, width, ndisp)

            # --views both: the right view is scored where the left one is and disp1GT.pfm exists (ListScorer.begin)
            truth = layout.load_truth(left_path) if self.scorer is not None else None
            truth_right = layout.load_truth_right(left_path) if (truth is not None and self.scorer.both) else None
            for t in (truth, truth_right):
                if t is not None:
                    evaluation.check_shape(t[0], (height, width), left_path)

            # decode + standardise (match.py:118-125): population std, no /255
            views = []
            for path in (left_path, right_path):
                g = util.read_gray(path).astype(np.float32)
                g = (g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1))
                views.append(np.expand_dims(g, axis=2))
            left_image, right_image = views
            if layout.kitti and right_image.shape != left_image.shape:
                raise ValueError("%s is %dx%d, the left view %dx%d" % (right_path, right_image.shape[1], right_image.shape[0],
                                                                       width, height))
            assert left_image.shape == (height, width, 1)
            assert right_image.shape == (height, width, 1)

            if len(self.pending) == in_flight:
                self.finish()                # the oldest pair is the one that used this slot
            self.launch(launched % in_flight, index, p, left_image, right_image, ndisp, truth, truth_right)
            if in_flight == 1:
                self.finish()
        while self.pending:
            self.finish()


def main(argv=None):
    args = parser.parse_args(argv)
    if args.fast and args.exact:
        parser.error("--fast and --exact exclude each other")
    if not 0 <= args.vertical_range <= 4:
        parser.error("--vertical_range: %d outside [0, 4]" % args.vertical_range)
    if args.vertical_range:
        for flag, on, why in (("--fast", args.fast, "the matrix-core cost volume has no vertical search"),
                              ("--separable_cbca", args.separable_cbca, "the vertical search writes pixel-major volumes, "
                               "the separable aggregation starts plane-major"),
                              ("--paper_support_regions", args.paper_support_regions, "the vertical search writes "
                               "pixel-major volumes, the two-view support regions start plane-major"),
                              ("--arch accurate", args.arch == "accurate", "the decision network has no vertical search")):
            if on:
                parser.error("--vertical_range is not available with %s: %s" % (flag, why))
    vertical_offset = parse_vertical_offset(args.vertical_offset)
    if vertical_offset is None:
        parser.error("--vertical_offset: %r is neither 'auto' nor an integer in [-8, 8], nor 'grid'" % args.vertical_offset)
    vertical_grid = parse_vertical_offset_grid(args.vertical_offset_grid)
    if vertical_grid is None:
        parser.error("--vertical_offset_grid: %r is not GHxGW with both in [1, 8]" % args.vertical_offset_grid)
    if not 1 <= args.vertical_offset_max <= 8:
        parser.error("--vertical_offset_max: %d outside [1, 8]" % args.vertical_offset_max)
    if args.vertical_offset_rows < 1:
        parser.error("--vertical_offset_rows: %d < 1" % args.vertical_offset_rows)
    if vertical_offset != 0:
        for flag, on, why in (("--fast", args.fast, "the matrix-core cost volume has no row offset"),
                              ("--separable_cbca", args.separable_cbca, "the offset cost volume writes pixel-major volumes, "
                               "the separable aggregation starts plane-major"),
                              ("--paper_support_regions", args.paper_support_regions, "the offset cost volume writes "
                               "pixel-major volumes, the two-view support regions start plane-major"),
                              ("--arch accurate", args.arch == "accurate", "the decision network has no row offset")):
            if on:
                parser.error("--vertical_offset is not available with %s: %s" % (flag, why))
    layout = datasets.get(args.dataset)
    try:
        eval_thresholds = layout.parse_thresholds(args.eval_thresholds if args.eval_thresholds is not None
                                                  else layout.default_thresholds)
    except ValueError as e:
        parser.error("--eval_thresholds: %s" % e)
    ndisp_flag = datasets.resolve_ndisp(layout, args.ndisp, parser.error)
    try:
        conf_names = parse_confidence(args.confidence)
    except ValueError as e:
        parser.error("--confidence: %s" % e)
    if args.eval_auc_threshold is not None and not (args.evaluate and conf_names):
        parser.error("--eval_auc_threshold goes with --evaluate --confidence")
    try:
        auc_threshold = layout.parse_auc_threshold(args.eval_auc_threshold if args.eval_auc_threshold is not None
                                                   else layout.default_auc_threshold)
    except ValueError as e:
        parser.error("--eval_auc_threshold: %s" % e)
    if args.eval_interpolate and not layout.kitti:
        parser.error("--eval_interpolate goes with a KITTI --dataset")
    eval_quantiles = None
    if args.eval_quantiles is not None:
        if not args.evaluate:
            parser.error("--eval_quantiles goes with --evaluate")
        if layout.kitti:
            parser.error("--eval_quantiles is not available with --dataset %s: the KITTI protocol has no error quantiles"
                         % args.dataset)
        try:
            eval_quantiles = evaluation.parse_quantiles(args.eval_quantiles)
        except ValueError as e:
            parser.error("--eval_quantiles: %s" % e)
    semi_rule = None
    if args.semi_dense is not None:
        if layout.kitti:
            parser.error("--semi_dense is not available with --dataset %s: the development kit's handling of sparse maps "
                         "is --eval_interpolate's" % args.dataset)
        try:
            semi_rule = SemiDenseRule.parse(args.semi_dense)
        except ValueError as e:
            parser.error("--semi_dense: %s" % e)
        missing = [n for n in semi_rule.measures if n not in conf_names]
        if missing:
            parser.error("--semi_dense reads the confidence measure %s, which --confidence does not name"
                         % ", ".join(missing))
    geometry = None
    if args.depth or args.point_cloud:
        if layout.kitti:
            parser.error("%s is not available with --dataset %s: the development kit's calibration format is not at hand"
                         % ("--depth" if args.depth else "--point_cloud", args.dataset))
        geometry = dict(depth=args.depth, points=args.point_cloud)
    if args.max_depth is not None:
        if not args.point_cloud:
            parser.error("--max_depth goes with --point_cloud")
        if args.max_depth != args.max_depth:
            parser.error("--max_depth: NaN")
        geometry["max_depth"] = args.max_depth
    calib_override = None
    if args.calib is not None:
        if geometry is None:
            parser.error("--calib goes with --depth or --point_cloud")
        try:
            calib_override = Calibration.parse(args.calib)
        except ValueError as e:
            parser.error("--calib: %s" % e)
    both = args.views == "both"
    if both and layout.kitti:
        parser.error("--views both is not available with --dataset %s: the KITTI development kit has neither right-view "
                     "ground truth nor a submission slot for a right map" % args.dataset)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    util.pin_gpu(args, world)     # before torch initialises HIP

    import torch
    import _hipabi as hip
    import stereo_device as sd
    from distributed import shard_indices
    from model import ACCURATE_NET, NET

    with open(args.list_file, "r") as f:
        left_paths = [line.strip() for line in f.readlines()]
    indices = shard_indices(args.start, args.end, len(left_paths), rank, world)
    if layout.kitti:
        # one --ndisp serves the whole list: a frame it does not fit (ndisp > W - 2) is refused here, from the image
        # headers, before the GPU is touched
        for index in indices:
            sd.check_envelope(*layout.shape(left_paths[index], ndisp_flag))

    hip.require_device()
    # one rank per GPU under torchrun; MCCNN_SHARED_GPU=1 (tests) lets several ranks share the visible GPUs
    shared = os.environ.get("MCCNN_SHARED_GPU") == "1"
    torch.cuda.set_device((local_rank % torch.cuda.device_count() if shared else local_rank) if world > 1 else 0)

    result_root = os.path.join(args.save_dir, "submit_{}".format(args.tag))        # match.py:69-72
    image_root = os.path.join(args.save_dir, "submit_{}_imgs".format(args.tag))
    util.recurMk(os.path.abspath(result_root))
    util.recurMk(os.path.abspath(image_root))

    accurate = args.arch == "accurate"
    if accurate:
        net = ACCURATE_NET(None, input_patch_size=args.patch_size, num_conv_layers=(args.patch_size - 1) // 2,
                           batch_size=1, device="cuda", num_fc_layers=args.num_fc_layers)
    else:
        net = NET(None, input_patch_size=args.patch_size, num_conv_layers=(args.patch_size - 1) // 2, batch_size=1,
                  device="cuda")
    net.restore(args.resume)  # loaded once and kept resident (the reference re-restores per pair)
    in_flight = max(1, int(args.pairs_in_flight))

    # --vertical_offset: the extras and the workspace keywords of the same names; nothing without the flag
    vertical_kw = dict(vertical_offset=vertical_offset, vertical_offset_max=args.vertical_offset_max,
                       vertical_offset_rows=args.vertical_offset_rows) if vertical_offset != 0 else {}
    if vertical_offset == "grid":
        vertical_kw["vertical_offset_grid"] = vertical_grid
    measured = vertical_offset in ("auto", "grid")      # the pair's measurement crosses and is written

    def save_vertical(offset, totals, out, field=None, cell_totals=None):
        """--vertical_offset auto | grid: the pair's measurement (host arrays) as verticalMCCNN.json."""
        record = sd.vertical_record(offset, totals) if field is None \
            else sd.vertical_field_record(offset, totals, field, cell_totals)
        record = dict(record, max_offset=args.vertical_offset_max, row_step=args.vertical_offset_rows)
        path = layout.vertical_path(out)
        util.recurMk(os.path.abspath(os.path.dirname(path)))
        with open(path, "w") as f:
            json.dump(record, f, sort_keys=True)
            f.write("\n")

    def make_matcher(features, decision=args.decision):
        return sd.StereoMatcher(
            net, hyper_parameters(args),
            cv_mode=hip.MCCNN_CV_MFMA if args.fast else hip.MCCNN_CV_EXACT,
            cbca_order=hip.MCCNN_CBCA_SEPARABLE if (args.fast and args.separable_cbca) else hip.MCCNN_CBCA_REFERENCE_ORDER,
            features=features, decision=decision,
            on_saturation="ignore",      # several pairs may be in flight: the loops poll the flag and repeat them
            extras=dict(both_view_support=args.paper_support_regions,
                        interpolation_directions=16 if args.paper_interpolation else 4,
                        occlusion_from_left=args.paper_interpolation, numpy1_promotion=args.numpy1_promotion,
                        sgm_independent_directions=args.paper_sgm, vertical_range=args.vertical_range, **vertical_kw),
            confidence=conf_names, views=args.views, semi_dense=semi_rule, geometry=geometry)

    def calibration(p):
        """--depth / --point_cloud: the pair's calibration, its calib.txt read by key unless --calib overrides it."""
        return calib_override if calib_override is not None else Calibration.from_middlebury(p["calib"])

    def save_geometry(result, out):
        """The left view's depth plane and cloud.  The whole record buffer crossed (nothing is read back to size the copy):
        the first n_points records are the cloud, in the device's order; a vertex takes its intensity from the grey left
        image through the record's pixel index."""
        if result.depth is not None:
            util.writePfm(result.depth, layout.depth_path(out))
        if result.points is not None:
            records = result.points[:int(np.asarray(result.n_points).view(np.uint32)[0])]
            grey = util.read_gray(out["left"]).reshape(-1)
            write_ply(layout.points_path(out), records, grey[point_pixels(records)])

    def save(result, out):
        """The files of a pair from the PairResult of host arrays that crossed: the map's (--views both: [2,H,W], the right
        map as disp1MCCNN.*), then one PFM per measure from the planes [K,H,W] (layout.confidence_path names the file;
        the right view's as conf1MCCNN_<measure>.pfm), then the sparse map's PFM (the right view's as disp1MCCNN_s.pfm)."""
        views = [(v, result.view(v, both)) for v in range(2 if both else 1)]
        for v, r in views:
            (layout.save_right if v else layout.save)(r.map, out)
        for v, r in views:
            for k, name in enumerate(conf_names if r.planes is not None else ()):
                path = layout.confidence_path(out, name, v) if both else layout.confidence_path(out, name)
                util.recurMk(os.path.abspath(os.path.dirname(path)))
                util.writePfm(r.planes[k], path)
        for v, r in views:
            if r.sparse is not None:
                util.writePfm(r.sparse, layout.sparse_path(out, v))
        save_geometry(result, out)

    def paths(index):
        # Middlebury: outputs mirror the input tree under the two roots (match.py:99-110): <root>/<dir of im0.png relative
        # to data_dir>; a KITTI layout: the development kit's submission tree (src/datasets.py)
        left_path = left_paths[index]
        return dict(layout.outputs(left_path, args.data_dir, result_root, image_root), left=left_path,
                    right=layout.right(left_path), calib=None if layout.kitti else layout.calib(left_path))

    matchers = [make_matcher("miopen" if args.features == "library" else "auto") for _ in range(in_flight)]
    footprint_kw = dict(pairs_in_flight=in_flight, arch=args.arch,
                        fc_units=net.num_fc_units if accurate else sd.DECISION_UNITS, confidence=len(conf_names),
                        views=args.views, **(dict(semi_dense=True) if semi_rule is not None else {}), **vertical_kw,
                        **(dict(depth=args.depth, points=args.point_cloud) if geometry is not None else {}))

    def footprint(height, width, ndisp):        # refuses a shape outside the envelope, with its message
        return sd.workspace_bytes(height, width, ndisp, matchers[0].pixel_major(),
                                  matchers[0].workspace_cbca_kernel(height, width, ndisp), **footprint_kw)

    def make_library_matcher():                 # the saturation redo's
        return make_matcher("miopen", "library")

    streams = [torch.cuda.Stream() for _ in range(in_flight)] if in_flight > 1 else [None]
    # --evaluate: one result buffer and scratch per slot, the list's running total on the device (src/evaluation.py)
    # (--views both: a second evaluator of the same kind, whose total pools the right maps against disp1GT.pfm)
    # (--eval_quantiles: both evaluators also select the error quantiles of every map and pool them over the list)
    # (--confidence: the sparsification figures of every scored map, behind its evaluation on its stream)
    scorer = None
    if args.evaluate:
        report = evaluation.ListReport(
            layout.evaluator(eval_thresholds, slots=in_flight, interpolate=args.eval_interpolate, quantiles=eval_quantiles),
            layout.evaluator(eval_thresholds, slots=in_flight, quantiles=eval_quantiles) if both else None,
            # (--semi_dense: one more evaluator per view, whose total pools the view's sparse maps; no quantiles)
            **(dict(semi=(semi_rule.describe(), layout.evaluator(eval_thresholds, slots=in_flight),
                          layout.evaluator(eval_thresholds, slots=in_flight) if both else None))
               if semi_rule is not None else {}))
        scorer = evaluation.ListScorer(report, evaluation.Sparsifier(conf_names, auc_threshold) if conf_names else None,
                                       args.views)
    eval_path = os.path.join(result_root, "eval.json" if world == 1 else "eval_rank{}.json".format(rank))
    pipeline = None
    if args.pipeline:
        backend = list_matcher.MatcherBackend(matchers, streams, make_library_matcher, rank=rank, scorer=scorer,
                                              device_output=layout.device_output if layout.kitti else None,
                                              vertical=measured)
        # (--depth / --point_cloud: the calibration joins the job's key - a graph is good for the calibration it was
        # captured with, so a pair is replayed only where shape AND calibration repeat; Middlebury's differ pair by pair)
        # a KITTI frame's size is its decoded left image's: the capture policy sees every change through the job's key
        reader = list_matcher.make_reader(
            paths, footprint, truth=layout.load_truth if args.evaluate else None,
            shape=(lambda left, image: layout.shape(left, ndisp_flag, image)) if layout.kitti else None,
            truth_right=layout.load_truth_right if (args.evaluate and both) else None,
            calibration=calibration if geometry is not None else None)
        writer = list_matcher.make_writer(rank, scorer=scorer, eval_file=out_eval_file, save=save,
                                          save_vertical=save_vertical if measured else None)
        pipeline = list_matcher.ListPipeline(reader, backend, writer, slots=in_flight, readers=args.readers)
        try:
            pipeline.run(indices)
        finally:
            print("[{}] {}".format(rank, pipeline.summary()))
    else:
        loop = ListLoop(layout, matchers, streams, sd.SaturationRedo(matchers, make_library_matcher), scorer, save, rank,
                        save_vertical=save_vertical if measured else None,
                        calibration=calibration if geometry is not None else None)
        loop.run(indices, paths, lambda left_path: layout.shape(left_path, ndisp_flag), footprint)
    if scorer is not None:
        scorer.report.write(eval_path)
    return pipeline


if __name__ == "__main__":
    main()


