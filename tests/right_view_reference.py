"""The right view's rules (include/mccnn.h: mccnn_lr_status_right, mccnn_interpolate_right, mccnn_confidence_right*) for
the tests, twice over.  No GPU, no fixtures.

  F-wrappers      the binding definition: the existing left-view restatements (post_reference, paper_rules_reference,
                  confidence_reference) applied to the horizontally flipped arrays, flipped back;
  literal loops   the rule spelled out in image coordinates, pixel by pixel, as the header states it - partner at
                  x + d, candidates d < min(W - x, D), occlusions from the left, rays that round half DOWN along x.

test_right_view_cpu.py asserts that the two agree on every case below, so that the flip identity itself is checked
where no GPU is needed; the GPU tests compare the kernels with the F-wrappers.  Expectations are computed once per case
(functools.lru_cache) and handed out read-only."""
import functools
import math
import warnings

import numpy as np

import confidence_reference as cr
import paper_rules_reference as ppr
import post_reference as pr

F32 = np.float32


def F(a):
    """The horizontal flip of a map [H,W] or a volume [D,H,W]: the last axis reversed, contiguous."""
    return np.array(np.asarray(a)[..., ::-1], order="C", copy=True)


# ---- the definition: left-view restatements on flipped arrays ---------------------------------------------------------
def lr_status_right(dr, dl, D):
    return F(pr.lr_status(F(dr), F(dl), D))


def interpolate_right(dr, status, directions=4, occlusion_from_right=False):
    """occlusion_from_right is the flipped frame's occlusion_from_left."""
    out = F(ppr.interpolate_ex(F(dr), F(status), directions, bool(occlusion_from_right)))
    if directions == 4 and not occlusion_from_right and out.shape[1] <= 300:
        # the reference's own rule has a second restatement (which lists a whole row per pixel: narrow maps only)
        other = F(pr.interpolate(F(dr), F(status)))
        assert np.array_equal(out.view(np.uint32), other.view(np.uint32))
    return out


def confidence_right(vol_right_dhw, disp_left, measures=15):
    """-> (planes [K,H,W], d1 [H,W]) of the right volume: confidence_reference.confidence on the flipped operands."""
    planes, d1 = cr.confidence(F(vol_right_dhw), None if disp_left is None else F(disp_left), measures)
    return F(planes), F(d1)


# ---- the rule in image coordinates, literally ----------------------------------------------------------------------
def lr_status_right_loop(dr, dl, D):
    dr, dl = np.ascontiguousarray(dr, F32), np.ascontiguousarray(dl, F32)
    H, W = dr.shape
    st = np.empty((H, W), np.int32)
    with np.errstate(invalid="ignore"):
        for h in range(H):
            for x in range(W):
                rf = dr[h, x]
                if not (rf > -1):
                    st[h, x] = 2
                    continue
                rd = int(rf)
                if x + rd > W - 1:
                    st[h, x] = 2
                    continue
                if abs(rd - dl[h, x + rd]) <= 1:
                    st[h, x] = 0
                    continue
                st[h, x] = 2
                for d in range(min(W - x, D)):
                    if abs(d - dl[h, x + d]) <= 1:
                        st[h, x] = 1
                        break
    return st


def interpolate_right_loop(dr, status, directions=4, occlusion_from_right=False):
    dr = np.ascontiguousarray(dr, F32)
    H, W = dr.shape
    st = np.asarray(status).tolist()
    out = dr.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for h in range(H):
            for w in range(W):
                s = st[h][w]
                if s == 1:
                    nb = []
                    if directions == 16:
                        for dx, dy in ppr.RAYS:
                            k = 0
                            while True:
                                k += 1
                                xi = int(math.ceil(w + k * (-dx) - 0.5))        # round half down
                                yi = int(math.floor(h + k * dy + 0.5))          # round half up
                                if xi < 0 or xi >= W or yi < 0 or yi >= H:
                                    break
                                if st[yi][xi] == 0:
                                    nb.append(dr[yi, xi])
                                    break
                    else:
                        for xs in (range(w - 1, -1, -1), range(w + 1, W)):       # left, right
                            for x in xs:
                                if st[h][x] == 0:
                                    nb.append(dr[h, x])
                                    break
                        for ys in (range(h + 1, H), range(h - 1, -1, -1)):       # below, above
                            for y in ys:
                                if st[y][w] == 0:
                                    nb.append(dr[y, w])
                                    break
                    if nb:
                        out[h, w] = np.median(np.array(nb, dtype=np.float32))
                elif s == 2:
                    for x in (range(w + 1, W) if occlusion_from_right else range(w - 1, -1, -1)):
                        if st[h][x] == 0:
                            out[h, w] = dr[h, x]
                            break
    return out


def lrc_right_loop(d1, disp_left):
    """The LRC plane of the right view from the winner map d1 [H,W] (int, -1: none) and the left map."""
    dl = np.ascontiguousarray(disp_left, F32)
    H, W = dl.shape
    out = np.full((H, W), -np.inf, F32)
    with np.errstate(invalid="ignore"):
        for h in range(H):
            for w in range(W):
                d = int(d1[h, w])
                if d < 0:
                    continue
                x = w + d
                if x > W - 1:
                    continue
                v = dl[h, x]
                if not (v >= F32(0.0)) or v == F32(np.inf):
                    continue
                out[h, w] = np.negative(np.abs(F32(F32(d) - v)))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (5, 1, 2), (2, 5, 3),                       # degenerate
          (3, 31, 8), (3, 32, 8), (3, 33, 8),                    # the 32-bit hit-mask word
          (3, 63, 16), (3, 64, 16), (3, 65, 16),                 # ballot and 64-bit word seams of the row kernel
          (2, 255, 40), (2, 256, 40), (2, 257, 40),              # the 256-thread stride
          (4, 70, 64), (2, 40, 64),                              # D > W
          (1, 1030, 1024),                                       # the largest D
          (1, 16385, 4)]                                         # the walk kernel and the row limit
MATCH_SHARES = (0.03, 0.5, 0.97)

# the seed of a (shape index, match-share index, special) case whose default (0) leaves one of the three states out;
# chosen on the CPU from the expected status alone (test_right_view_cpu.py asserts the condition on every case)
SEEDS = {}


def shape_id(s):
    return "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def lr_case(si, mi, special):
    """(dr, dl, expected status) of one case: post_reference.make_lr_maps at the shape with the roles swapped -
    dr = F(dl0), dl = F(dr0) - so that the map being judged carries the left map's edge values."""
    H, W, D = SHAPES[si]
    seed = SEEDS.get((si, mi, bool(special)), 0)
    rng = np.random.default_rng([23, si, mi, int(special), seed])
    dl0, dr0 = pr.make_lr_maps(H, W, D, rng, MATCH_SHARES[mi], bool(special))
    dr, dl = F(dl0), F(dr0)
    want = lr_status_right(dr, dl, D)
    for a in (dr, dl, want):
        a.setflags(write=False)
    return dr, dl, want


def lr_cases(si):
    for mi in range(len(MATCH_SHARES)):
        for special in (False, True):
            yield (mi, special) + lr_case(si, mi, special)


def all_states_expected(si):
    H, W, _ = SHAPES[si]
    return H * W >= 12


# interpolation: the status kinds of paper_rules_reference plus a single match in the first column (the mirror of
# corner_match's single match in the last); "all_mismatch" is the all-unmatched map, "odd_words" has words besides 0/1/2
STATUS_KINDS = ppr.STATUS_KINDS + ("first_column_match",)
MAP_KINDS = ppr.MAP_KINDS
MODES = [(4, False), (4, True), (16, False), (16, True)]          # (directions, occlusion_from_right)
# kinds whose restatement walks a whole row from every pixel: quadratic in W, left out above this width (the kernels
# take no other path for them there than at 257 columns - several mask words, more than one 256-thread stride - where
# they are all run)
WALK_HEAVY = ("all_mismatch", "corner_match", "first_column_match")
WALK_HEAVY_MAX_W = 300


def status_kinds_for(W):
    return tuple(k for k in STATUS_KINDS if W <= WALK_HEAVY_MAX_W or k not in WALK_HEAVY)


def map_kinds_for(W):
    """Indices into MAP_KINDS: both value classes, above 4096 columns "special" alone (it holds every value the other
    has besides its own; the restatement's cost is per pixel)."""
    return (0, 1) if W <= 4096 else (1,)


@functools.lru_cache(maxsize=None)
def interp_inputs(si, ki, mi):
    H, W, _ = SHAPES[si]
    kind = STATUS_KINDS[ki]
    rng = np.random.default_rng([29, si, ki, mi])
    dr = ppr.disparity_map(MAP_KINDS[mi], H, W, rng)
    if kind == "first_column_match":
        st = F(ppr.status_map("corner_match", H, W, rng))
        st = np.ascontiguousarray(st[::-1])                      # the match at (0, 0)
    else:
        st = ppr.status_map(kind, H, W, rng)
    dr.setflags(write=False)
    st.setflags(write=False)
    return dr, st


@functools.lru_cache(maxsize=None)
def interp_expected(si, ki, mi, directions, occ):
    dr, st = interp_inputs(si, ki, mi)
    want = interpolate_right(dr, st, directions, occ)
    want.setflags(write=False)
    return want


# confidence: confidence_reference.make_volume kinds at these shapes; the left map is built for the RIGHT winners
CONF_SHAPES = [(1, 4, 2), (3, 9, 5), (7, 11, 16), (2, 300, 257), (1, 1030, 1024)]
CONF_KINDS = ("normal", "quant")


def make_left_map(vol_right_dhw, seed):
    """A left map for a right volume: confidence_reference.make_right_map in the flipped frame (mostly the winner of the
    pixel it is read from, +-1, fractions, and the special values scattered over it)."""
    return F(cr.make_right_map(F(vol_right_dhw), seed))


@functools.lru_cache(maxsize=None)
def conf_case(ci, ki):
    """(right volume [D,H,W], left map, planes of all four measures, d1).  The volume is make_volume's with its columns
    reversed, so that its single-pixel edits (forced winners 0 and D-1, ties, all-NaN pixels) keep their places in the
    flipped frame, and the pixels of the last column win at every d1, d1 > 0 included: x + d1 > W-1."""
    H, W, D = CONF_SHAPES[ci]
    vol = F(cr.make_volume(H, W, D, CONF_KINDS[ki], seed=H * 1000 + W + D + 7))
    vol[-1, :, W - 1] = F32(-60.0)                                # the last column's winner is D-1 (unless NaN / -inf)
    left = make_left_map(vol, seed=D + 1)
    planes, d1 = confidence_right(vol, left, 15)
    for a in (vol, left, planes, d1):
        a.setflags(write=False)
    return vol, left, planes, d1


def planes_of(want_all, mask):
    return np.stack([want_all[cr.plane_index(15, n)] for n in cr.NAMES if mask & cr.BITS[n]])


def names_of(mask):
    return tuple(n for n in cr.NAMES if mask & cr.BITS[n])


# ---- the whole right view behind the winner-take-all maps -------------------------------------------------------------
def post_right(right_image, dl, dr, vol_right_dhw, D, hp=None, extras=None):
    """{stage: map} of the right view under the names StereoMatcher's keep= uses, from the two winner-take-all maps, the
    final right volume and the right image: the mirrored check and interpolation, then the oracle's (view-agnostic)
    sub-pixel, median and bilateral stages on the right view's operands."""
    import oracle as o
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    ex = dict(ppr.EXTRAS_OFF)
    ex.update(extras or {})
    st = lr_status_right(dr, dl, D)
    di = interpolate_right(dr, st, ex["interpolation_directions"], ex["occlusion_from_left"])
    ds = ppr.subpixel_numpy1(di, vol_right_dhw) if ex["numpy1_promotion"] else o.subpixel_enhance(di, vol_right_dhw)
    dm = o.median_filter(ds, 5, 5)
    db = o.bilateral_filter(right_image, dm, 5, 5, 0, a["blur_sigma"], a["blur_threshold"])
    return dict(status_right=st, interp_right=di, subpixel_right=ds, median_right=dm, bilateral_right=db)


RIGHT_STAGES = ("status_right", "interp_right", "subpixel_right", "median_right", "bilateral_right")
