"""Patch sampler for training the matching network - drop-in for /root/reference/src/datagenerator.py
(ImageDataGenerator, :13-240): same constructor arguments, attributes and methods, NumPy only.

A mini-batch is drawn from ONE stereo pair (datagenerator.py:137-216): `batch_size` pixels with a finite, non-occluded
ground-truth disparity; for each one the left patch centred on it, a positive right patch centred within
`dataset_pos` pixels of the true match and a negative one displaced by `dataset_neg_low .. dataset_neg_high` pixels to
either side.  Patches are cut from images zero-padded by (patch-1)/2, so border pixels are legal centres.

Differences a maintainer should know:
  * images are decoded by util.read_gray (PIL + libpng's grey conversion, pinned in tests) instead of cv2;
  * the per-pixel Python loops are replaced by vectorised draws with the same distributions and the same rejection
    rules (int() truncation of the displaced column, redraw until it lies inside the image); the stream of random
    numbers is therefore not the reference's - pass `rng` (a numpy Generator) for reproducible batches.

DevicePatchSampler (not in the reference) keeps the images on the GPU and cuts every batch there with one HIP launch:
the reference's rule bit for bit (sampling="pair"), or the paper's - one shuffled pool of every valid pixel, fractional
centres, data set augmentation.  The index drawing of a pair's batch is the module-level draw_pair_centres, which both
classes call.
"""
import numpy as np

from util import read_gray, readPfm


def displaced_columns(right_col, width, draw, truncate=True):
    """right_col + deviation, redrawn per sample until it lies inside the image (:199-212).  truncate: the reference's
    int(right_col + deviation) (towards zero), an integer column; otherwise the fractional column is kept (float64) and
    must lie in [0, width - 1].  `width` is one number or one per sample; draw(n) returns n deviations."""
    col = np.full(right_col.shape, -1, dtype=np.int64 if truncate else np.float64)
    todo = np.ones(right_col.shape, dtype=bool)
    while todo.any():
        dev = draw(int(todo.sum()))
        if truncate:
            col[todo] = np.trunc(right_col[todo] + dev).astype(np.int64)     # Python int(): towards zero
            todo = (col < 0) | (col >= width)
        else:
            col[todo] = right_col[todo] + dev
            todo = (col < 0) | (col > np.asarray(width) - 1)
    return col


def draw_displaced(rng, right_col, width, dataset_pos, dataset_neg_low, dataset_neg_high, truncate=True):
    """The positive and the negative column of every sample (:189-212): within dataset_pos of the true match, and
    dataset_neg_low .. dataset_neg_high away from it on either side.  All positives are drawn before all negatives."""
    pos_col = displaced_columns(right_col, width, lambda n: rng.uniform(-1 * dataset_pos, dataset_pos, size=n), truncate)

    def neg_dev(n):
        dev = rng.uniform(dataset_neg_low, dataset_neg_high, size=n)
        return np.where(rng.integers(-1, 1, size=n) == -1, -dev, dev)

    neg_col = displaced_columns(right_col, width, neg_dev, truncate)
    return pos_col, neg_col


def draw_pair_centres(rng, gt_image, batch_size, dataset_pos, dataset_neg_low, dataset_neg_high, truncate=True):
    """The index drawing of one mini-batch from one pair (:155-212): (rows, cols, pos_col, neg_col), the left centres
    and the columns of the positive and the negative right patch on the same rows.  ImageDataGenerator.next_batch and
    DevicePatchSampler's pair mode both call it: it IS the order in which `rng` is consumed.  truncate=False keeps the
    fractional disparity and the fractional displaced columns (float64) instead of the reference's int(), and a pixel is
    then valid when gt <= col (not int(gt) <= col), so that the true match lies inside the image."""
    height, width = gt_image.shape
    # distinct rows and distinct columns first (:161-162), then redraw the samples that land on an unknown
    # (inf) or occluded (match left of the image) pixel anywhere in the image (:165-170)
    rows = rng.permutation(height)[:batch_size].astype(np.int64)
    cols = rng.permutation(width)[:batch_size].astype(np.int64)
    assert len(rows) == batch_size and len(cols) == batch_size, "batch_size exceeds the image height or width"

    def invalid(r, c):
        g = gt_image[r, c]
        bad = np.isinf(g)
        known = np.where(bad, 0, g)
        # the match must not lie left of the image: int(gt) <= col, or gt <= col where the fraction is kept - a match
        # at col - gt in (-1, -0.5] would leave the positive's interval [col - gt - pos, col - gt + pos] outside the
        # image, and its redraw would never end
        bad |= (np.trunc(known) if truncate else known) > c
        return bad

    bad = invalid(rows, cols)
    while bad.any():
        n = int(bad.sum())
        rows[bad] = rng.integers(0, height, size=n)
        cols[bad] = rng.integers(0, width, size=n)
        bad = invalid(rows, cols)

    g = gt_image[rows, cols]
    right_col = cols - np.trunc(g).astype(np.int64) if truncate else cols - g.astype(np.float64)
    pos_col, neg_col = draw_displaced(rng, right_col, width, dataset_pos, dataset_neg_low, dataset_neg_high, truncate)
    return rows, cols, pos_col, neg_col


class ImageDataGenerator(object):

    def __init__(self, left_image_list_file, shuffle=False, patch_size=(11, 11), in_left_suffix='im0.png',
                 in_right_suffix='im1.png', gt_suffix='disp0GT.pfm', dataset_neg_low=1.5, dataset_neg_high=6,
                 dataset_pos=0.5, rng=None, layout=None):
        # layout: a datasets.py layout whose path mapping and ground-truth reader replace the three suffixes (None: the
        # reference's suffix replacement and PFM reader)
        self.layout = layout
        self.shuffle = shuffle
        self.patch_size = patch_size
        self.in_left_suffix = in_left_suffix
        self.in_right_suffix = in_right_suffix
        self.gt_suffix = gt_suffix
        self.dataset_neg_low = dataset_neg_low
        self.dataset_neg_high = dataset_neg_high
        self.dataset_pos = dataset_pos
        self.rng = rng if rng is not None else np.random.default_rng()
        self.pointer = 0          # which pair the next batch comes from (datagenerator.py:44-46)
        self.read_image_list(left_image_list_file)
        self.prefetch()
        if self.shuffle:
            self.shuffle_data()

    def read_image_list(self, image_list):
        """Right-view and ground-truth paths follow from the left path by suffix replacement (:54-70)."""
        with open(image_list) as f:
            self.left_paths = [line.strip() for line in f if line.strip()]
        if self.layout is not None:
            self.right_paths = [self.layout.right(p) for p in self.left_paths]
            self.gt_paths = [self.layout.truth_paths(p)[-1] for p in self.left_paths]
        else:
            self.right_paths = [p.replace(self.in_left_suffix, self.in_right_suffix) for p in self.left_paths]
            self.gt_paths = [p.replace(self.in_left_suffix, self.gt_suffix) for p in self.left_paths]
        self.data_size = len(self.left_paths)

    @staticmethod
    def _standardise(gray_u8):
        img = gray_u8.astype(np.float32) / 255.                       # :85 (training divides by 255, matching does not;
        return (img - np.mean(img, axis=(0, 1))) / np.std(img, axis=(0, 1))   # standardisation removes the factor)

    def prefetch(self):
        """All pairs are kept in memory (:73-97): stereo training sets are a few dozen images."""
        self.left_images = [self._standardise(read_gray(p)) for p in self.left_paths]
        self.right_images = [self._standardise(read_gray(p)) for p in self.right_paths]
        if self.layout is not None:      # float32, +inf where unknown, whatever the files hold (KITTI: kitti_gt_to_float)
            self.gt_images = [np.asarray(self.layout.load_truth_float(p), dtype=np.float32) for p in self.left_paths]
        else:
            self.gt_images = [np.asarray(readPfm(p), dtype=np.float32) for p in self.gt_paths]

    def shuffle_data(self):
        order = self.rng.permutation(self.data_size)
        for name in ("left_paths", "right_paths", "gt_paths", "left_images", "right_images", "gt_images"):
            setattr(self, name, [getattr(self, name)[i] for i in order])

    def reset_pointer(self):
        self.pointer = 0
        if self.shuffle:
            self.shuffle_data()

    def _padded(self, image):
        ph, pw = self.patch_size
        out = np.zeros((image.shape[0] + ph - 1, image.shape[1] + pw - 1), dtype=np.float32)
        out[(ph - 1) // 2:(ph - 1) // 2 + image.shape[0], (pw - 1) // 2:(pw - 1) // 2 + image.shape[1]] = image
        return out

    def _cut(self, padded, rows, cols):
        """[B, ph, pw, 1] patches whose top-left corners in the padded image are (rows, cols) = centred on the pixel."""
        ph, pw = self.patch_size
        rr = rows[:, None, None] + np.arange(ph)[None, :, None]
        cc = cols[:, None, None] + np.arange(pw)[None, None, :]
        return padded[rr, cc][..., None].astype(np.float32)

    def _displaced(self, right_col, width, draw):
        """int(right_col + deviation), redrawn per sample until it lies inside the image (:199-212)."""
        return displaced_columns(right_col, width, draw)

    def next_batch(self, batch_size):
        left_image = self.left_images[self.pointer]
        right_image = self.right_images[self.pointer]
        gt_image = self.gt_images[self.pointer]
        assert left_image.shape == right_image.shape
        assert left_image.shape[0:2] == gt_image.shape
        rows, cols, pos_col, neg_col = draw_pair_centres(self.rng, gt_image, batch_size, self.dataset_pos,
                                                         self.dataset_neg_low, self.dataset_neg_high)
        pl, pr = self._padded(left_image), self._padded(right_image)
        patches_left = self._cut(pl, rows, cols)
        patches_right_pos = self._cut(pr, rows, pos_col)
        patches_right_neg = self._cut(pr, rows, neg_col)
        self.pointer += 1
        return patches_left, patches_right_pos, patches_right_neg

    def next_pair(self):
        i = self.pointer
        assert self.left_images[i].shape == self.right_images[i].shape
        assert self.left_images[i].shape[0:2] == self.gt_images[i].shape
        self.pointer += 1
        return self.left_images[i], self.right_images[i], self.gt_images[i]


# ---- the device-side sampler: pooled sampling, augmented patches, one HIP launch per batch -----------------------------

# include/mccnn.h: mccnn_sample_t (36 bytes) and mccnn_sample_image_t (16 bytes)
SAMPLE_DTYPE = np.dtype([("image", "<i4"), ("cy", "<f4"), ("cx", "<f4"), ("m", "<f4", (4,)), ("gain", "<f4"),
                         ("bias", "<f4")])
SAMPLE_IMAGE_DTYPE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4")])
assert SAMPLE_DTYPE.itemsize == 36 and SAMPLE_IMAGE_DTYPE.itemsize == 16

AUGMENT_KEYS = ("rotate", "scale", "hscale", "hshear", "trans", "brightness", "contrast", "d_rotate", "d_hscale",
                "d_hshear", "d_vtrans", "d_brightness", "d_contrast")
# The paper's table of augmentation hyperparameters (Zbontar & LeCun 2016, "Data set augmentation"), QUOTED FROM MEMORY:
# the paper is not at hand where this was written, so the values are unverified (PAPERS.md says the same).  Check them
# against the paper before relying on them; every one can be overridden (train.py --aug_<key>).
AUGMENT_MIDDLEBURY = dict(rotate=28, scale=0.8, hscale=0.8, hshear=0.1, trans=0, brightness=1.3, contrast=1.1,
                          d_rotate=3, d_hscale=0.9, d_hshear=0.3, d_vtrans=1, d_brightness=0.7, d_contrast=1.1)
AUGMENT_KITTI = dict(rotate=7, scale=1, hscale=0.9, hshear=0.1, trans=0, brightness=0.7, contrast=1.3,
                     d_rotate=0, d_hscale=1, d_hshear=0, d_vtrans=0, d_brightness=0.3, d_contrast=1)
AUGMENT_NONE = dict(rotate=0, scale=1, hscale=1, hshear=0, trans=0, brightness=0, contrast=1, d_rotate=0, d_hscale=1,
                    d_hshear=0, d_vtrans=0, d_brightness=0, d_contrast=1)


def augment_matrix(sx, sy, sh, phi):
    """[..., 2, 2] float64: the forward map from source offsets to patch offsets (x first),
    A = Shear(sh) . Rot(phi) . diag(sx, sy), Rot(phi) = [[cos, sin], [-sin, cos]], Shear(sh) = [[1, sh], [0, 1]]."""
    sx, sy, sh, phi = (np.asarray(a, dtype=np.float64) for a in (sx, sy, sh, phi))
    c, s = np.cos(phi), np.sin(phi)
    # Shear . Rot = [[c - sh*s, s + sh*c], [-s, c]]
    return np.stack([np.stack([(c - sh * s) * sx, (s + sh * c) * sy], -1), np.stack([-s * sx, c * sy], -1)], -2)


def _inverse_2x2(a):
    det = a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0]
    inv = np.stack([np.stack([a[..., 1, 1], -a[..., 0, 1]], -1), np.stack([-a[..., 1, 0], a[..., 0, 0]], -1)], -2)
    return inv / det[..., None, None] + 0.0          # + 0.0: an identity map has no -0.0 entries


class DevicePatchSampler(ImageDataGenerator):
    """Mini-batches cut on the GPU: the standardised left and right images of every pair of the list live in ONE flat
    device float32 pool (left then right per pair, unpadded: image 2p and 2p + 1), a batch is drawn on the host as 3B
    sample records - lefts, positives, negatives, the order Trainer.loss stacks - and one launch of
    mccnn_sample_patches (csrc/sample.hip) turns them into the [3B, ps, ps, 1] device tensor the network reads.
    Ground truth stays on the host.  device=None builds everything except the device buffers (draw() works, next_batch()
    does not): there is no CPU fallback for the cut.

    sampling="pair": the reference's rule, one pair per batch; the same `rng` calls in the same order as
      ImageDataGenerator.next_batch, identity records - the same seed gives the same patches, bit for bit.
    sampling="pool": the paper's rule.  Every valid (pair, row, col) of the list (finite ground truth, int(gt) <= col)
      goes into one table with its disparity and width; one permutation of it per epoch, consecutive slices of B; steps_per_epoch =
      n_valid // batch_size (// world_size: under torchrun every rank permutes with its own seed), the remainder is
      dropped; reset_pointer() draws the next permutation.
    truncate=True keeps the reference's int() of the disparity and of the displaced right columns; False keeps both
      fractional (the paper's rule: centres are floats here), the redraw rule applied to the fractional column; a pixel
      is then valid when gt <= col, the reference's int(gt) <= col on the un-truncated disparity.
    augment: None or a dict of AUGMENT_KEYS (missing keys: no effect), drawn in float64 per triplet, in this order:
        s = U(scale, 1); sx = s * U(hscale, 1); sy = s; sh = U(-hshear, hshear); tx, ty = U(-trans, trans) each;
        phi = U(-rotate, rotate) deg; b = U(-brightness, brightness); k = U(1/contrast, contrast)
      and, shared by the positive and the negative right patch,
        sx' = sx * U(d_hscale, 1); sh' = sh + U(-d_hshear, d_hshear); ty' = ty + U(-d_vtrans, d_vtrans);
        phi' = phi + U(-d_rotate, d_rotate) deg; b' = b + U(-d_brightness, d_brightness);
        k' = k * U(1/d_contrast, d_contrast).
      The record carries m = float32(inverse of augment_matrix(sx, sy, sh, phi)) (inverted in float64), the centre
      minus t, gain k and bias b.  After draw(), `last_params` holds the drawn quantities and `last_records` the records.
    """

    def __init__(self, left_image_list_file, shuffle=False, patch_size=(11, 11), in_left_suffix='im0.png',
                 in_right_suffix='im1.png', gt_suffix='disp0GT.pfm', dataset_neg_low=1.5, dataset_neg_high=6,
                 dataset_pos=0.5, rng=None, device="cuda", sampling="pair", truncate=True, augment=None, batch_size=128,
                 world_size=1, layout=None):
        if sampling not in ("pair", "pool"):
            raise ValueError("sampling must be 'pair' or 'pool', not %r" % (sampling,))
        if patch_size[0] != patch_size[1] or patch_size[0] < 1 or patch_size[0] % 2 == 0 or patch_size[0] > 31:
            raise ValueError("the device sampler cuts square patches of odd side up to 31, not %r" % (patch_size,))
        if augment is not None:
            unknown = sorted(set(augment) - set(AUGMENT_KEYS))
            if unknown:
                raise ValueError("unknown augmentation keys %s" % unknown)
            augment = dict(AUGMENT_NONE, **augment)
        self.sampling = sampling
        self.truncate = truncate
        self.augment = augment
        self.batch_size = int(batch_size)         # of steps_per_epoch; draw() and next_batch() take their own
        self.world_size = max(1, int(world_size))
        self.device = device
        self.last_records = None
        self.last_params = None
        self.order = None
        ImageDataGenerator.__init__(self, left_image_list_file, shuffle=shuffle and sampling == "pair",
                                    patch_size=patch_size, in_left_suffix=in_left_suffix,
                                    in_right_suffix=in_right_suffix, gt_suffix=gt_suffix, dataset_neg_low=dataset_neg_low,
                                    dataset_neg_high=dataset_neg_high, dataset_pos=dataset_pos, rng=rng, layout=layout)
        if sampling == "pool":
            self._build_valid_table()
            self._next_permutation()
        if device is not None:
            self._upload()

    # -- the image pool ----------------------------------------------------------------------------------------------
    def prefetch(self):
        self._load_images()
        self._build_pool()

    def _load_images(self):
        ImageDataGenerator.prefetch(self)

    def _build_pool(self):
        self.order = np.arange(self.data_size)     # position in the epoch -> pair of the list (shuffle_data permutes it)
        table = np.zeros(2 * self.data_size, dtype=SAMPLE_IMAGE_DTYPE)
        offset = 0
        for p in range(self.data_size):
            assert self.left_images[p].shape == self.right_images[p].shape
            assert self.left_images[p].shape[0:2] == self.gt_images[p].shape
            for k, img in enumerate((self.left_images[p], self.right_images[p])):
                table[2 * p + k] = (offset, img.shape[0], img.shape[1])
                offset += img.size
        pool = np.empty(offset, dtype=np.float32)
        for k, img in enumerate(x for pair in zip(self.left_images, self.right_images) for x in pair):
            pool[table["offset"][k]:table["offset"][k] + img.size] = img.ravel()
        for p in range(self.data_size):            # the host images become views of the pool: one copy in memory
            for k, images in enumerate((self.left_images, self.right_images)):
                t = table[2 * p + k]
                images[p] = pool[t["offset"]:t["offset"] + t["H"] * t["W"]].reshape(t["H"], t["W"])
        self.pool_host, self.image_table = pool, table

    def _upload(self):
        import torch
        import _hipabi as hip
        hip.load()
        self.device = torch.device(self.device)
        if self.device.type != "cuda":
            raise hip.MccnnHipError("DevicePatchSampler cuts on the GPU; there is no CPU fallback (device=None builds "
                                    "the host side alone)")
        self.pool = torch.from_numpy(self.pool_host).to(self.device)
        self.images_dev = torch.from_numpy(self.image_table.view(np.uint8)).to(self.device)
        self._ring, self._ring_at, self._records_dev = [], 0, None

    def shuffle_data(self):
        """The permutation ImageDataGenerator.shuffle_data draws, kept as an index: the pool is not reordered."""
        self.order = self.order[self.rng.permutation(self.data_size)]

    # -- pool mode ---------------------------------------------------------------------------------------------------
    def _build_valid_table(self):
        """Every valid (pair, row, col) of the list with its disparity and its image's width: finite ground truth and
        int(gt) <= col, the reference's rule - or gt <= col with truncate=False, the same rule on the un-truncated
        disparity (draw_pair_centres says why)."""
        pairs, rows, cols, gts, widths = [], [], [], [], []
        for p, gt in enumerate(self.gt_images):
            finite = np.isfinite(gt)
            known = np.where(finite, gt, 0)
            ok = finite & ((np.trunc(known) if self.truncate else known) <= np.arange(gt.shape[1])[None, :])
            r, c = np.nonzero(ok)
            pairs.append(np.full(r.shape, p, dtype=np.int32))
            rows.append(r.astype(np.int32))
            cols.append(c.astype(np.int32))
            gts.append(gt[r, c].astype(np.float32))
            widths.append(np.full(r.shape, gt.shape[1], dtype=np.int32))
        self.valid_pair, self.valid_row, self.valid_col, self.valid_gt, self.valid_width = (
            np.concatenate(a) for a in (pairs, rows, cols, gts, widths))
        self.n_valid = len(self.valid_pair)

    def _next_permutation(self):
        self._perm = self.rng.permutation(self.n_valid)
        self._cursor = 0

    @property
    def steps_per_epoch(self):
        """Batches in one epoch: the pairs of the list, or n_valid // batch_size in pool mode (per rank)."""
        if self.sampling == "pair":
            return self.data_size
        return self.n_valid // self.batch_size // self.world_size

    def reset_pointer(self):
        self.pointer = 0
        if self.sampling == "pool":
            self._next_permutation()
        elif self.shuffle:
            self.shuffle_data()

    def next_pair(self):
        i = self.order[self.pointer]
        self.pointer += 1
        return self.left_images[i], self.right_images[i], self.gt_images[i]

    # -- drawing -----------------------------------------------------------------------------------------------------
    def _draw_centres(self, batch_size):
        """(pair, rows, cols, pos_col, neg_col) of the next batch; advances the pointer."""
        args = (self.dataset_pos, self.dataset_neg_low, self.dataset_neg_high, self.truncate)
        if self.sampling == "pair":
            p = int(self.order[self.pointer])
            rows, cols, pos_col, neg_col = draw_pair_centres(self.rng, self.gt_images[p], batch_size, *args)
            pair = np.full(batch_size, p, dtype=np.int64)
        else:
            if self._cursor + batch_size > self.n_valid:
                raise IndexError("the epoch's permutation is used up: reset_pointer() draws the next one")
            idx = self._perm[self._cursor:self._cursor + batch_size]
            self._cursor += batch_size
            pair, rows, cols = (a[idx].astype(np.int64) for a in (self.valid_pair, self.valid_row, self.valid_col))
            g, width = self.valid_gt[idx], self.valid_width[idx].astype(np.int64)
            right_col = cols - np.trunc(g).astype(np.int64) if self.truncate else cols - g.astype(np.float64)
            pos_col, neg_col = draw_displaced(self.rng, right_col, width, *args)
        self.pointer += 1
        return pair, rows, cols, pos_col, neg_col

    def _draw_augmentation(self, B):
        a, rng = self.augment, self.rng

        def U(lo, hi):
            return rng.uniform(lo, hi, size=B)

        q = {}
        q["s"] = U(a["scale"], 1)
        q["sx"] = q["s"] * U(a["hscale"], 1)
        q["sy"] = q["s"]
        q["sh"] = U(-a["hshear"], a["hshear"])
        q["tx"], q["ty"] = U(-a["trans"], a["trans"]), U(-a["trans"], a["trans"])
        q["phi"] = U(-a["rotate"], a["rotate"]) * np.pi / 180
        q["b"] = U(-a["brightness"], a["brightness"])
        q["k"] = U(1. / a["contrast"], a["contrast"])
        q["sx_r"] = q["sx"] * U(a["d_hscale"], 1)
        q["sh_r"] = q["sh"] + U(-a["d_hshear"], a["d_hshear"])
        q["ty_r"] = q["ty"] + U(-a["d_vtrans"], a["d_vtrans"])
        q["phi_r"] = q["phi"] + U(-a["d_rotate"], a["d_rotate"]) * np.pi / 180
        q["b_r"] = q["b"] + U(-a["d_brightness"], a["d_brightness"])
        q["k_r"] = q["k"] * U(1. / a["d_contrast"], a["d_contrast"])
        return q

    def draw(self, batch_size):
        """The 3B records of the next batch as a SAMPLE_DTYPE array: B lefts, B positives, B negatives."""
        B = batch_size
        pair, rows, cols, pos_col, neg_col = self._draw_centres(B)
        rec = np.zeros(3 * B, dtype=SAMPLE_DTYPE)
        cy = np.tile(rows.astype(np.float64), 3)
        cx = np.concatenate([cols, pos_col, neg_col]).astype(np.float64)
        rec["image"] = np.concatenate([2 * pair, 2 * pair + 1, 2 * pair + 1])
        rec["m"] = (1, 0, 0, 1)
        rec["gain"] = 1
        self.last_params = None
        if self.augment is not None:
            q = self._draw_augmentation(B)
            m_left = _inverse_2x2(augment_matrix(q["sx"], q["sy"], q["sh"], q["phi"])).reshape(B, 4)
            m_right = _inverse_2x2(augment_matrix(q["sx_r"], q["sy"], q["sh_r"], q["phi_r"])).reshape(B, 4)
            rec["m"] = np.concatenate([m_left, m_right, m_right]).astype(np.float32)
            cx = cx - np.tile(q["tx"], 3)
            cy = cy - np.concatenate([q["ty"], q["ty_r"], q["ty_r"]])
            rec["gain"] = np.concatenate([q["k"], q["k_r"], q["k_r"]])
            rec["bias"] = np.concatenate([q["b"], q["b_r"], q["b_r"]])
            self.last_params = q
        rec["cy"], rec["cx"] = cy, cx
        # the kernel trusts the image index and cannot report an error: refuse here, before the upload
        if ((rec["image"] < 0) | (rec["image"] >= len(self.image_table))).any():
            raise ValueError("a sample record names an image outside the pool of %d" % len(self.image_table))
        if not (np.isfinite(rec["cy"]).all() and np.isfinite(rec["cx"]).all()):
            raise ValueError("a sample record has a centre that is not finite")
        self.last_records = rec
        return rec

    # -- the cut -----------------------------------------------------------------------------------------------------
    def cut(self, records):
        """[N, ps, ps, 1] device tensor: one launch of mccnn_sample_patches on the current stream.  The records go up
        through a ring of pinned buffers with a non-blocking copy; the call does not wait for the device."""
        import torch
        import _hipabi as hip
        if self.device is None:
            raise hip.MccnnHipError("DevicePatchSampler(device=None) cannot cut: there is no CPU fallback")
        n, nbytes, ps = len(records), records.nbytes, self.patch_size[0]
        if self._records_dev is None or self._records_dev.numel() < nbytes:
            self._records_dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ring = [[torch.empty(nbytes, dtype=torch.uint8).pin_memory(), None] for _ in range(4)]
        slot = self._ring[self._ring_at]
        self._ring_at = (self._ring_at + 1) % len(self._ring)
        if slot[1] is not None:
            slot[1].synchronize()                   # the copy out of this buffer, four batches ago, has been made
        slot[0][:nbytes].copy_(torch.from_numpy(np.ascontiguousarray(records).view(np.uint8)))
        self._records_dev[:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        out = torch.empty((n, ps, ps, 1), dtype=torch.float32, device=self.device)
        hip.check(hip.load().mccnn_sample_patches(hip.ptr(self.pool), hip.ptr(self.images_dev), len(self.image_table),
                                                  hip.ptr(self._records_dev), n, ps, hip.ptr(out), hip.stream()),
                  "mccnn_sample_patches")
        return out

    def next_batch(self, batch_size):
        """[3B, ps, ps, 1] device tensor of the next batch (lefts, positives, negatives): what Trainer.step_stacked reads."""
        return self.cut(self.draw(batch_size))
