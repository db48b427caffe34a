"""Data set layouts: where the files of a stereo pair are and what is in them.

match.py, train.py and the list pipeline ask one object the same questions about a pair, whatever the data set:

    right(left)                       the right view's path
    truth_paths(left)                 the ground-truth files (one or two)
    load_truth(left)                  what the evaluator of this layout takes, or None without a ground-truth file
    load_truth_float(left)            float32 [H,W], +inf where unknown: Middlebury's convention, for training
    shape(left, ndisp, left_image)    (H, W, ndisp) of the pair
    outputs(left, data_dir, result_root, image_root)   the output paths, and the directories they need
    device_output(map) / save(...)    what crosses to the host for a map (and what is scored), and the files written from it
    evaluator(...)                    the evaluation.Evaluator that scores this layout's truth

`middlebury` is what match.py and train.py did before they knew of layouts, behind this interface: im0.png / im1.png /
calib.txt / disp0GT.pfm / mask0nocc.png in one directory per pair, float32 PFM out.

`kitti2015` and `kitti2012` are the development kits' trees, from memory of them: a list entry is
.../image_2/NNNNNN_10.png (2015) or .../colored_0/NNNNNN_10.png or .../image_0/NNNNNN_10.png (2012); the right view is the
same file under image_3 (colored_1, image_1), the ground truth under disp_occ_0 and disp_noc_0 (2012: disp_occ, disp_noc)
as 16-bit PNGs - 0 is "no value", anything else the disparity times 256.  Size comes from the decoded left image, ndisp
from the command line (the paper's 228 unless told otherwise).  The truth stays uint16 to the device
(mccnn_evaluate_kitti reads it as it is: half the bytes of a float map); the map is encoded to the same 16-bit code on the
device (mccnn_kitti_encode_u16) and only that plane crosses to the host; an evaluation scores what the PNG holds
(mccnn_kitti_decode_u16 of the plane), so its figures are the file's.
"""
import os

import numpy as np

import util

KITTI_NDISP = 228     # the paper's disparity range on KITTI


def kitti_gt_to_float(code):
    """KITTI's uint16 disparity code as Middlebury's float map: v / 256 (exact in float32), 0 -> +inf."""
    code = np.asarray(code)
    if code.dtype != np.uint16:
        raise ValueError("expected a uint16 plane, got %s" % code.dtype)
    out = code.astype(np.float32) / np.float32(256.0)
    out[code == 0] = np.inf
    return out


class Middlebury(object):
    name = "middlebury"
    kitti = False
    left_suffix, right_suffix, calib_suffix, gt_suffix = "im0.png", "im1.png", "calib.txt", "disp0GT.pfm"
    out_file, out_img_file, out_time_file, out_eval_file = "disp0MCCNN.pfm", "disp0MCCNN.pgm", "timeMCCNN.txt", "evalMCCNN.json"
    default_thresholds = "0.5,1,2,4"
    # match.py --views both: the right view's map, preview and ground truth (Middlebury ships disp1GT.pfm / mask1nocc.png)
    right_gt_suffix, right_out_file, right_out_img_file = "disp1GT.pfm", "disp1MCCNN.pfm", "disp1MCCNN.pgm"

    def right(self, left):
        return left.replace(self.left_suffix, self.right_suffix)

    def load_truth_right(self, left):
        """load_truth() of the RIGHT view: disp1GT.pfm / mask1nocc.png beside the left image, or None."""
        import evaluation
        return evaluation.load_ground_truth(left, view="right")

    def save_right(self, disparity, paths):
        util.saveDisparity(disparity, paths["out_img_right"])
        util.writePfm(disparity, paths["out_right"])

    def calib(self, left):
        return left.replace(self.left_suffix, self.calib_suffix)

    def truth_paths(self, left):
        return (left.replace(self.left_suffix, self.gt_suffix),)

    def load_truth(self, left):
        import evaluation
        return evaluation.load_ground_truth(left)

    def load_truth_float(self, left):
        return np.asarray(util.readPfm(self.truth_paths(left)[0]), dtype=np.float32)

    def shape(self, left, ndisp=None, left_image=None):
        return util.parseCalib(self.calib(left))

    def outputs(self, left, data_dir, result_root, image_root):
        pair_dir = os.path.dirname(left)
        res_dir = pair_dir.replace(data_dir, result_root)
        img_dir = pair_dir.replace(data_dir, image_root)
        return dict(res_dir=res_dir, img_dir=img_dir, dirs=(res_dir, img_dir), out=os.path.join(res_dir, self.out_file),
                    out_time=os.path.join(res_dir, self.out_time_file), out_img=os.path.join(img_dir, self.out_img_file),
                    out_eval=os.path.join(res_dir, self.out_eval_file),
                    out_right=os.path.join(res_dir, self.right_out_file),
                    out_img_right=os.path.join(img_dir, self.right_out_img_file))

    def parse_thresholds(self, text):
        import evaluation
        return evaluation.parse_thresholds(text)

    default_auc_threshold = "1.0"

    def parse_auc_threshold(self, text):
        """--eval_auc_threshold: one error in pixels; a pixel is bad when err > T."""
        import evaluation
        values = evaluation.parse_thresholds(text)
        if len(values) != 1:
            raise ValueError("expected one threshold, got %r" % (text,))
        return values[0]

    def confidence_path(self, paths, measure, view=0):
        """match.py --confidence: the plane of `measure` beside disp0MCCNN.pfm (view 1, --views both: conf1MCCNN_*)."""
        return os.path.join(paths["res_dir"], "conf%dMCCNN_%s.pfm" % (int(view), measure))

    def sparse_path(self, paths, view=0):
        """match.py --semi_dense: the sparse map beside disp0MCCNN.pfm, named as Middlebury's sparse track names it (view
        1, --views both: disp1MCCNN_s.pfm)."""
        return os.path.join(paths["res_dir"], "disp%dMCCNN_s.pfm" % int(view))

    def depth_path(self, paths):
        """match.py --depth: the left view's depth plane beside disp0MCCNN.pfm, unknown pixels as inf."""
        return os.path.join(paths["res_dir"], "depth0MCCNN.pfm")

    def points_path(self, paths):
        """match.py --point_cloud: the left view's point cloud beside disp0MCCNN.pfm."""
        return os.path.join(paths["res_dir"], "points0MCCNN.ply")

    def vertical_path(self, paths):
        """match.py --vertical_offset auto: the pair's measured row offset beside disp0MCCNN.pfm."""
        return os.path.join(paths["res_dir"], "verticalMCCNN.json")

    def evaluator(self, thresholds, slots=1, interpolate=False, device=None, quantiles=None):
        import evaluation
        return evaluation.Evaluator(device, thresholds, slots, quantiles=quantiles)

    def device_output(self, disparity, scored=False):
        """(what crosses to the host for a map, the map an evaluation scores): both the map itself."""
        return disparity, disparity

    def save(self, disparity, paths):
        util.saveDisparity(disparity, paths["out_img"])
        util.writePfm(disparity, paths["out"])


class Kitti(object):
    kitti = True

    def __init__(self, name, views, truth, map_dir, default_thresholds):
        self.name = name
        self.views = views                    # (left directory, right directory) alternatives
        self.truth = truth                    # (occ directory, noc directory)
        self.map_dir = map_dir                # of the submission tree
        self.default_thresholds = default_thresholds

    def _sibling(self, left, directory):
        view_dir, name = os.path.split(left)
        return os.path.join(os.path.dirname(view_dir), directory, name)

    def right(self, left):
        view = os.path.basename(os.path.dirname(left))
        for left_dir, right_dir in self.views:
            if view == left_dir:
                return self._sibling(left, right_dir)
        raise ValueError("%s: a %s list names left images under %s, not under %r"
                         % (left, self.name, " or ".join(l for l, _ in self.views), view))

    def truth_paths(self, left):
        self.right(left)                      # refuses a path outside the layout
        return tuple(self._sibling(left, d) for d in self.truth)

    def load_truth(self, left):
        """(disp_occ uint16 [H,W], disp_noc uint16 [H,W] or None), or None without a disp_occ file."""
        occ_path, noc_path = self.truth_paths(left)
        if not os.path.isfile(occ_path):
            return None
        occ = util.read_u16(occ_path)
        noc = util.read_u16(noc_path) if os.path.isfile(noc_path) else None
        if noc is not None and noc.shape != occ.shape:
            raise ValueError("%s is %s, %s is %s" % (noc_path, noc.shape, occ_path, occ.shape))
        return occ, noc

    def load_truth_float(self, left):
        """The non-occluded truth where there is one (what the paper trains on), else the occluded."""
        occ_path, noc_path = self.truth_paths(left)
        return kitti_gt_to_float(util.read_u16(noc_path if os.path.isfile(noc_path) else occ_path))

    def shape(self, left, ndisp=None, left_image=None):
        if left_image is None:
            from PIL import Image
            with Image.open(left) as im:
                width, height = im.size
        else:
            height, width = left_image.shape[:2]
        return int(height), int(width), int(ndisp if ndisp is not None else KITTI_NDISP)

    def outputs(self, left, data_dir, result_root, image_root):
        stem = os.path.splitext(os.path.basename(left))[0]
        res_dir = os.path.join(result_root, self.map_dir) if self.map_dir else result_root
        img_dir = os.path.dirname(left).replace(data_dir, image_root)
        time_dir, eval_dir = os.path.join(result_root, "time"), os.path.join(result_root, "eval")
        return dict(res_dir=res_dir, img_dir=img_dir, dirs=(res_dir, img_dir, time_dir, eval_dir),
                    out=os.path.join(res_dir, stem + ".png"), out_time=os.path.join(time_dir, stem + ".txt"),
                    out_img=os.path.join(img_dir, stem + ".pgm"), out_eval=os.path.join(eval_dir, stem + ".json"))

    def parse_thresholds(self, text):
        import evaluation
        return evaluation.parse_kitti_thresholds(text)

    default_auc_threshold = "3:0.05"

    def parse_auc_threshold(self, text):
        """--eval_auc_threshold: one abs[:rel] item; a pixel is bad when err > abs and err > rel * truth."""
        import evaluation
        pairs = evaluation.parse_kitti_thresholds(text)
        if len(pairs) != 1:
            raise ValueError("expected one abs[:rel] threshold, got %r" % (text,))
        return pairs[0]

    def confidence_path(self, paths, measure):
        """match.py --confidence: submit_<tag>/conf_<measure>/NNNNNN_10.pfm (the submission tree's root is where its
        time/ directory hangs)."""
        root = os.path.dirname(os.path.dirname(paths["out_time"]))
        stem = os.path.splitext(os.path.basename(paths["out"]))[0]
        return os.path.join(root, "conf_%s" % measure, stem + ".pfm")

    def vertical_path(self, paths):
        """match.py --vertical_offset auto: submit_<tag>/vertical/NNNNNN_10.json."""
        root = os.path.dirname(os.path.dirname(paths["out_time"]))
        stem = os.path.splitext(os.path.basename(paths["out"]))[0]
        return os.path.join(root, "vertical", stem + ".json")

    def evaluator(self, thresholds, slots=1, interpolate=False, device=None, quantiles=None):
        import evaluation
        return evaluation.KittiEvaluator(device, thresholds, slots, interpolate, quantiles=quantiles)

    def device_output(self, disparity, scored=False):
        """(the 16-bit plane that crosses to the host and becomes the PNG, the map an evaluation scores: what that PNG
        holds, decoded on the device - the figures are those of the file, as the development kit would compute them; None
        unless `scored`).  Two launches behind the map on the current stream."""
        import stereo_device
        code = stereo_device.kitti_encode_u16(disparity)
        return code, (stereo_device.kitti_decode_u16(code) if scored else None)

    def save(self, code, paths):
        """The 16-bit PNG, and the 8-bit preview of what that PNG holds (0 where it holds no value)."""
        util.write_png_u16(code, paths["out"])
        util.saveDisparity(code.astype(np.float32) / np.float32(256.0), paths["out_img"])


LAYOUTS = {
    "middlebury": Middlebury(),
    "kitti2015": Kitti("kitti2015", (("image_2", "image_3"),), ("disp_occ_0", "disp_noc_0"), "disp_0", "3:0.05"),
    "kitti2012": Kitti("kitti2012", (("colored_0", "colored_1"), ("image_0", "image_1")), ("disp_occ", "disp_noc"), "",
                       "2,3,4,5"),
}
NAMES = tuple(LAYOUTS)


def get(name):
    return LAYOUTS[name]


def resolve_ndisp(layout, ndisp, error):
    """--ndisp belongs to the KITTI layouts (Middlebury's comes from calib.txt): error(message) otherwise."""
    if not layout.kitti:
        if ndisp is not None:
            error("--ndisp goes with a KITTI --dataset: a Middlebury pair's ndisp comes from its calib.txt")
        return None
    ndisp = KITTI_NDISP if ndisp is None else int(ndisp)
    if ndisp < 1:
        error("--ndisp must be positive")
    return ndisp
