"""GPU: cost_volume_mfma_kernel (csrc/cost_volume.hip, MCCNN_CV_MFMA, the cost volume of `--fast`) against the float64
dot product, on features whose scores are where the argmin looks - true matches with <fl, fr> near 1 - and not only on
independent Gaussian vectors, whose scores and therefore whose rounding errors are the smallest there are.

Numerics, over ALL scored entries (w >= d) of both volumes (tests/fast_kernels_reference.py has the families):
  * |got - scores64| <= tolerances.COST_VOLUME_MFMA_ABS, the stated contract;
  * E_mfma <= COST_VOLUME_MFMA_E32_FACTOR * E32 + 2^-24, E32 being the error of the CPU oracle's float32 pairwise sum on
    the same inputs - a bound that comes from the reference's side, never from the kernel;
  * the families whose scores are exactly representable come back exactly (the sign of a zero is not pinned).
Borders: the w < d / x >= W - d entries are what mccnn_cost_volume_fill (bit-pinned elsewhere) makes of the kernel's own
scores.  Stores: outputs start as a sentinel; the Dp - D pads of the pixel-major volumes and a guard plane either side
of the plane-major ones still hold it; two calls give the same bits; both layouts hold the same bits; a refused call
writes nothing.  NaN: a NaN feature marks exactly the entries it marks in the exact mode.

The measured E_mfma, E32 and their ratio per family and shape go to parity_cost_volume_mfma.json in the directory
MCCNN_RECORD_DIR names (profiles/parity_cost_volume_mfma.json is a copy)."""
import json
import os

import numpy as np
import pytest
import torch

import fast_kernels_reference as R
import tolerances as tol

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
SENTINEL_BITS = SENTINEL.view(np.uint32)

# (H, W, D): what each one reaches first (64 x 64 tiles, bands of 64 disparities, the folded product tile's ragged quads,
# the XCD work order)
SHAPES = [
    (1, 10, 2),                                             # fewer than 8 workgroups
    (2, 63, 5), (2, 64, 4), (2, 65, 61), (2, 66, 64),       # D = W - 2, one band
    (2, 130, 64), (2, 132, 130),                            # a last band with 2 disparities, Dp > D
    (3, 131, 2), (2, 193, 65),
    (2, 260, 256),
    (1, 750, 256),                                          # the benchmark's width
]
ALL_FAMILY_SHAPES = [(2, 130, 64), (2, 260, 256)]
EVERY_SHAPE_FAMILIES = ("gauss", "matched_0", "nonneg")
ALL_FAMILIES = ("gauss", "matched_0", "matched_3", "antiparallel", "near", "nonneg", "wide", "golden", "onehot", "eighths")
CASES = [(s, f) for s in SHAPES for f in (ALL_FAMILIES if s in ALL_FAMILY_SHAPES else EVERY_SHAPE_FAMILIES)]


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def record_measured(record):
    out = os.environ.get("MCCNN_RECORD_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "parity_cost_volume_mfma.json")
        old = {}
        if os.path.isfile(path):
            with open(path) as f:
                old = json.load(f)
        old.update(record)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


_families, _reference = {}, {}


def families(H, W):
    if (H, W) not in _families:
        fams = R.feature_families(H, W, seed=H * 10000 + W)
        for pair in fams.values():
            for f in pair:
                f.setflags(write=False)
        _families[(H, W)] = fams
    return _families[(H, W)]


def reference(key, fl, fr, D):
    """(left64, right64, mask_left, mask_right, E32) of one case, computed once on the CPU and handed out read-only.  The
    masks leave out entries whose float64 score is NaN (a NaN feature): those are compared as a set."""
    if key not in _reference:
        import oracle as o
        with np.errstate(invalid="ignore"):
            left, right, ml, mr = R.scores64(fl, fr, D)
            ol, orr = o.compute_cost_volume(fl, fr, D)
        ml, mr = ml & ~np.isnan(left), mr & ~np.isnan(right)
        e32 = max(float(np.abs(ol[ml] - left[ml]).max()), float(np.abs(orr[mr] - right[mr]).max()))
        for a in (left, right, ml, mr):
            a.setflags(write=False)
        _reference[key] = (left, right, ml, mr, e32)
    return _reference[key]


def run_hwd(sd, fl, fr, D, mode):
    """mccnn_cost_volume_hwd into sentinel-filled buffers -> two device tensors [H, W, Dp]."""
    import _hipabi as hip
    H, W, _ = fl.shape
    out = tuple(torch.full((H, W, sd.hwd_pitch(D)), float(SENTINEL), device="cuda") for _ in range(2))
    sd.cost_volume_hwd(fl, fr, D, out=out, mode=hip.MCCNN_CV_MFMA if mode == "mfma" else hip.MCCNN_CV_EXACT)
    return out


def run_planes(sd, fl, fr, D):
    """mccnn_cost_volume(MCCNN_CV_MFMA) into the middle of sentinel-filled [D + 2, H, W] buffers -> the two buffers."""
    import _hipabi as hip
    H, W, _ = fl.shape
    bufs = tuple(torch.full((D + 2, H, W), float(SENTINEL), device="cuda") for _ in range(2))
    sd.cost_volume(fl, fr, D, mode=hip.MCCNN_CV_MFMA, out=tuple(b[1:D + 1] for b in bufs))
    return bufs


def check_numerics(got_l, got_r, ref, family, what):
    """got_*: host [D, H, W].  Returns the measured record."""
    left, right, ml, mr, e32 = ref
    with np.errstate(invalid="ignore"):
        el, er = np.abs(got_l.astype(np.float64) - left), np.abs(got_r.astype(np.float64) - right)
    assert not np.isnan(el[ml]).any() and not np.isnan(er[mr]).any(), "%s: NaN among scores of NaN-free pixels" % what
    e = max(float(el[ml].max()), float(er[mr].max()))
    bound = tol.COST_VOLUME_MFMA_E32_FACTOR * e32 + 2.0 ** -24
    print("%s: E_mfma %.3e  E32 %.3e  ratio %s  relative bound %.3e" % (what, e, e32, "%.2f" % (e / e32) if e32 else "-", bound))
    assert e <= tol.COST_VOLUME_MFMA_ABS, "%s: %g from the float64 dot product, the contract is %g" % (
        what, e, tol.COST_VOLUME_MFMA_ABS)
    assert e <= bound, "%s: E_mfma %g > %d * E32 (%g) + 2^-24" % (what, e, tol.COST_VOLUME_MFMA_E32_FACTOR, e32)
    if family in R.EXACT_FAMILIES:
        assert e32 == 0 and e == 0, "%s: exactly representable scores came back inexact (%g)" % (what, e)
    return {"E_mfma": e, "E32": e32, "ratio": e / e32 if e32 else None, "entries": int(ml.sum() + mr.sum())}


def to_planes(t, D):
    return np.ascontiguousarray(t.cpu().numpy()[:, :, :D].transpose(2, 0, 1))


def border_masks(H, W, D, Dp):
    """[H, W, Dp] bool: the entries of the left / right pixel-major volume that the border fill owns."""
    w, d = np.arange(W)[None, :, None], np.arange(Dp)[None, None, :]
    shape = (H, W, Dp)
    return np.broadcast_to((w < d) & (d < D), shape), np.broadcast_to((w >= W - d) & (d < D), shape)


@pytest.mark.parametrize("shape,family", CASES, ids=["%dx%dx%d-%s" % (s + (f,)) for s, f in CASES])
def test_pixel_major_against_float64(sd, shape, family):
    H, W, D = shape
    fl_np, fr_np = families(H, W)[family]
    got = run_hwd(sd, dev(fl_np), dev(fr_np), D, "mfma")
    host = [t.cpu().numpy() for t in got]
    what = "%s %dx%dx%d" % (family, H, W, D)
    rec = check_numerics(to_planes(got[0], D), to_planes(got[1], D), reference((shape, family), fl_np, fr_np, D), family, what)
    record_measured({"hwd %s" % what: rec})
    # the pads (d >= D) were never written
    for side, g in zip(("left", "right"), host):
        pad = g[:, :, D:]
        assert pad.size == 0 or bool((pad.view(np.uint32) == SENTINEL_BITS).all()), "%s volume: a pad entry was written" % side
    # the borders are the fill kernel's recurrences on the kernel's own scores
    Dp = host[0].shape[2]
    masks = border_masks(H, W, D, Dp)
    again = []
    for g, m in zip(host, masks):
        c = g.copy()
        c[m] = SENTINEL
        again.append(dev(c))
    sd.cost_volume_fill(again[0], again[1], D, True)
    for side, g, a, m in zip(("left", "right"), host, again, masks):
        a = a.cpu().numpy()
        assert np.array_equal(a.view(np.uint32), g.view(np.uint32)), "%s volume: borders are not the fill of the scores" % side
        assert D == 1 or not (g[m].view(np.uint32) == SENTINEL_BITS).any(), "%s volume: a border entry was left unwritten" % side


@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_plane_major_against_float64_and_pixel_major(sd, family):
    """mccnn_cost_volume(MCCNN_CV_MFMA): the folded product tile and its ragged quads.  Same bounds; the guard planes in
    front of and behind the volumes stay untouched; the bits are those of the pixel-major volumes."""
    H, W, D = 2, 130, 64
    fl_np, fr_np = families(H, W)[family]
    fl, fr = dev(fl_np), dev(fr_np)
    bufs = run_planes(sd, fl, fr, D)
    hwd = run_hwd(sd, fl, fr, D, "mfma")
    what = "%s %dx%dx%d" % (family, H, W, D)
    planes = [b[1:D + 1] for b in bufs]
    rec = check_numerics(planes[0].cpu().numpy(), planes[1].cpu().numpy(),
                         reference(((H, W, D), family), fl_np, fr_np, D), family, "plane-major " + what)
    record_measured({"dhw %s" % what: rec})
    for side, b, p, q in zip(("left", "right"), bufs, planes, hwd):
        guards = b[[0, D + 1]].cpu().numpy()
        assert bool((guards.view(np.uint32) == SENTINEL_BITS).all()), "%s volume: a guard plane was written" % side
        moved = sd.dhw_to_hwd(p.contiguous()).cpu().numpy()[:, :, :D]
        assert np.array_equal(moved.view(np.uint32), q.cpu().numpy()[:, :, :D].view(np.uint32)), \
            "%s volume: plane-major and pixel-major bits differ" % side


@pytest.mark.parametrize("family", ["matched_0", "gauss"])
def test_two_calls_are_bit_identical(sd, family):
    H, W, D = 2, 260, 256
    fl, fr = (dev(f) for f in families(H, W)[family])
    a, b = run_hwd(sd, fl, fr, D, "mfma"), run_hwd(sd, fl, fr, D, "mfma")
    pa, pb = run_planes(sd, fl, fr, D), run_planes(sd, fl, fr, D)
    for x, y in zip(a + pa, b + pb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_refused_calls_write_nothing(sd):
    import _hipabi as hip
    lib = hip.load()
    MFMA = hip.MCCNN_CV_MFMA
    #        H, W,    C,  D,    mode, pixel-major, expected
    cases = [(2, 50, 64, 64, MFMA, True, hip.MCCNN_E_UNSUPPORTED),        # D > W - 2
             (2, 50, 64, 64, MFMA, False, hip.MCCNN_E_UNSUPPORTED),
             (2, 130, 64, 129, MFMA, True, hip.MCCNN_E_UNSUPPORTED),
             (1, 1030, 64, 1025, MFMA, True, hip.MCCNN_E_UNSUPPORTED),    # D > 1024 (_hwd)
             (2, 130, 32, 16, MFMA, True, hip.MCCNN_E_UNSUPPORTED),       # C != 64
             (2, 130, 32, 16, MFMA, False, hip.MCCNN_E_UNSUPPORTED),
             (2, 130, 64, 16, 7, True, hip.MCCNN_E_INVALID),              # unknown mode
             (2, 130, 64, 16, 7, False, hip.MCCNN_E_INVALID)]
    for H, W, C, D, mode, pixel_major, want in cases:
        fl = torch.rand((H, W, C), device="cuda")
        fr = torch.rand((H, W, C), device="cuda")
        shape = (H, W, sd.hwd_pitch(D)) if pixel_major else (D, H, W)
        out = tuple(torch.full(shape, float(SENTINEL), device="cuda") for _ in range(2))
        fn = lib.mccnn_cost_volume_hwd if pixel_major else lib.mccnn_cost_volume
        rc = fn(hip.ptr(fl), hip.ptr(fr), H, W, C, D, hip.ptr(out[0]), hip.ptr(out[1]), mode, hip.stream())
        assert rc == want, (H, W, C, D, mode, pixel_major, rc)
        torch.cuda.synchronize()
        for t in out:
            assert bool((t == float(SENTINEL)).all()), "a refused call wrote to its output: %r" % ((H, W, C, D, mode),)


def test_nan_features_mark_the_entries_they_mark_in_the_exact_mode(sd):
    """A NaN in one channel of about 5 % of the pixels of each view (no inf).  The exact mode returns NaN for every score
    of such a pixel and for every border entry those scores reach; so does the matrix-core mode, in both layouts - the
    clamp in front of the f16 split lets NaN pass - and every score of two NaN-free pixels obeys the numeric bounds."""
    H, W, D = 2, 130, 64
    fl_np, fr_np = R.with_nans(*families(H, W)["gauss"], seed=9)
    assert 3 <= np.isnan(fl_np).any(-1).sum() <= 40 and not np.isinf(fl_np).any() and not np.isinf(fr_np).any()
    fl, fr = dev(fl_np), dev(fr_np)
    exact = [t.cpu().numpy()[:, :, :D] for t in run_hwd(sd, fl, fr, D, "exact")]
    got = run_hwd(sd, fl, fr, D, "mfma")
    planes = [b[1:D + 1].cpu().numpy() for b in run_planes(sd, fl, fr, D)]
    ref = reference("nan", fl_np, fr_np, D)
    scored_nan = int((~ref[2]).sum() - (~R.scores64(*families(H, W)["gauss"], D)[2]).sum())
    assert scored_nan > 500, "the inputs put too few NaN scores into the volume"
    for side, e, g, p in zip(("left", "right"), exact, got, planes):
        g = g.cpu().numpy()[:, :, :D]
        assert np.isnan(e).sum() >= scored_nan
        missing, extra = int((np.isnan(e) & ~np.isnan(g)).sum()), int((~np.isnan(e) & np.isnan(g)).sum())
        assert missing == 0 and extra == 0, "%s volume: %d entries are NaN in the exact mode and finite here, %d the " \
                                            "other way round" % (side, missing, extra)
        assert np.array_equal(np.isnan(p), np.isnan(e.transpose(2, 0, 1))), "%s volume, plane-major" % side
    rec = check_numerics(to_planes(got[0], D), to_planes(got[1], D), ref, "gauss", "gauss with NaN %dx%dx%d" % (H, W, D))
    check_numerics(planes[0], planes[1], ref, "gauss", "plane-major gauss with NaN %dx%dx%d" % (H, W, D))
    record_measured({"hwd gauss with NaN %dx%dx%d" % (H, W, D): rec})
