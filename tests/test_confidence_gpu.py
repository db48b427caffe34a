"""GPU: mccnn_confidence_hwd and mccnn_confidence through the C interface, bit for bit (helpers.assert_bits: uint32
patterns, NaN payloads canonicalised) against the literal restatement of tests/confidence_reference.py, at the smallest
shapes where the kernels can go wrong:

  (1,4,2), (2,5,3)            curvature at both ends with D = 2 and 3
  (3,9,4), (3,9,5)            pitch 4 and 8; the pad lanes hold -inf on one run and NaN on another and must not show
  (7,11,16)                   77 pixels: tails of the 8-pixel round and of the 64-pixel wave
  H*W = 1, 63, 64, 65         the smallest image and the 64-pixel wave boundary
  (5,67,64)                   one group of 256 disparities, partly filled
  (2,300,255 / 256 / 257)     the 256-disparity group seam
  (1,1030,1024)               the envelope's largest disparity count

confidence_reference.make_volume / make_right_map state the contents.  The restatement runs once per volume with all
four measures; a launch with fewer measures must reproduce the planes of those measures, in bit order."""
import numpy as np
import pytest
import torch

import confidence_reference as ref
from helpers import assert_bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 2), (2, 5, 3), (3, 9, 4), (3, 9, 5), (7, 11, 16), (1, 1, 8), (7, 9, 8), (8, 8, 8), (5, 13, 8), (5, 67, 64),
          (2, 300, 255), (2, 300, 256), (2, 300, 257), (1, 1030, 1024)]
MASKS = [ref.MSM, ref.MMN, ref.CUR, ref.LRC, 15]
CANARY = np.float32(-12345.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def names(mask):
    return tuple(n for n in ref.NAMES if mask & ref.BITS[n])


def planes_of(want_all, mask):
    return np.stack([want_all[ref.plane_index(15, n)] for n in names(mask)])


def run(entry, vol, D, right, mask):
    """One launch into the first K planes of a K + 1 plane buffer; the last plane is the canary."""
    import stereo_device as sd
    k = bin(mask).count("1")
    H, W = right.shape
    buf = torch.full((k + 1, H, W), float(CANARY), dtype=torch.float32, device="cuda")
    dr = right if mask & ref.LRC else None
    if entry == "hwd":
        got = sd.confidence_hwd(vol, D, dr, names(mask), out=buf[:k])
    else:
        got = sd.confidence(vol, dr, names(mask), out=buf[:k])
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert (host[k] == CANARY).all(), "the plane behind the %d requested ones was written" % k
    return host[:k]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("kind", ["normal", "quant"])
def test_both_entries_against_the_restatement(shape, kind):
    H, W, D = shape
    vol = ref.make_volume(H, W, D, kind, seed=H * 1000 + W + D)
    right = ref.make_right_map(vol, seed=D)
    want, d1 = ref.confidence(vol, right, 15)
    if H * W >= 60:                   # the contents are what the docstring says
        assert (d1 == -1).any() and (d1 == 0).any() and (d1 == D - 1).any()
        assert ((np.arange(W)[None, :] - d1 < 0) & (d1 >= 0)).any(), "no pixel with w - d1 < 0"
        assert np.isnan(want[1]).any() and (want[1] == 0).any() and (want[3] == -np.inf).any() and (want[3] == 0).any()
    dright, dvol = dev(right), dev(vol)
    for pad in (-np.inf, np.nan):
        hwd = dev(ref.to_hwd(vol, pad))
        for mask in MASKS:
            got = run("hwd", hwd, D, dright, mask)
            assert_bits(got, planes_of(want, mask), "mccnn_confidence_hwd %s %s pad %s measures %d" % (shape, kind, pad, mask))
    for mask in MASKS:
        got = run("dhw", dvol, D, dright, mask)
        assert_bits(got, planes_of(want, mask), "mccnn_confidence %s %s measures %d" % (shape, kind, mask))


def test_every_subset_in_bit_order():
    """All 15 selections on one volume: K = popcount planes, in ascending bit order, whatever order the names come in."""
    import stereo_device as sd
    H, W, D = 7, 11, 16
    vol = ref.make_volume(H, W, D, "normal", seed=5)
    right = ref.make_right_map(vol, seed=6)
    want, _ = ref.confidence(vol, right, 15)
    hwd, dvol, dright = dev(ref.to_hwd(vol, np.nan)), dev(vol), dev(right)
    for mask in range(1, 16):
        for entry, v in (("hwd", hwd), ("dhw", dvol)):
            assert_bits(run(entry, v, D, dright, mask), planes_of(want, mask), "%s measures %d" % (entry, mask))
    got = sd.confidence_hwd(hwd, D, dright, ("lrc", "msm")).cpu().numpy()
    assert_bits(got, planes_of(want, ref.MSM | ref.LRC), "names out of order")


def test_golden_pairs(golden_cases):
    """The reference's own final left volume and right map: the planes equal the restatement, the winner the stored
    wta_l."""
    for name, g in golden_cases:
        vol, right = g["cbca2_l"], g["wta_r"]
        D = vol.shape[0]
        want, d1 = ref.confidence(vol, right, 15)
        assert np.array_equal(d1.astype(np.float32), g["wta_l"])
        assert_bits(run("hwd", dev(ref.to_hwd(vol, np.nan)), D, dev(right), 15), want, name + " pixel-major")
        assert_bits(run("dhw", dev(vol), D, dev(right), 15), want, name + " plane-major")


def test_refusals_with_device_pointers():
    """The refusals that need real pointers to be told apart from a null one: overlap of out and disp_right."""
    import _hipabi as hip
    lib = hip.load()
    H, W, D = 4, 6, 4
    vol = torch.zeros((H, W, 4), device="cuda")
    buf = torch.zeros((5, H, W), device="cuda")
    st = hip.stream()
    for fn in (lib.mccnn_confidence_hwd, lib.mccnn_confidence):
        assert fn(hip.ptr(vol), hip.ptr(buf[1]), D, H, W, 15, hip.ptr(buf), st) == hip.MCCNN_E_INVALID
        assert b"overlaps" in lib.mccnn_last_error_string()
        assert fn(hip.ptr(vol), hip.ptr(buf[0]), D, H, W, 1, hip.ptr(buf[0]), st) == hip.MCCNN_E_INVALID
        assert fn(hip.ptr(vol), hip.ptr(buf[4]), D, H, W, 15, hip.ptr(buf), st) == 0
    torch.cuda.synchronize()
