"""GPU: the device-side ingest (mccnn_ingest_u8 / _pair through the C ABI) against NumPy's own expression, bit for bit;
StereoMatcher.match_u8 / match_graph_u8 against match() on the host-standardised images."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import ingest_helpers as ih

pytestmark = pytest.mark.gpu


def _ingest_abi(images, pair):
    """images: one or two uint8 arrays of one shape -> float32 outputs through the raw C ABI (no host wrapper)."""
    import torch
    import _hipabi as hip
    lib = hip.load()
    H, W = images[0].shape[:2]
    C = 1 if images[0].ndim == 2 else images[0].shape[2]
    dev = [torch.from_numpy(np.array(a, order="C")).cuda() for a in images]
    outs = [torch.full((H, W), -7.0, dtype=torch.float32, device="cuda") for _ in images]
    nbytes = int(lib.mccnn_ingest_scratch_bytes(H, W))
    scratch = torch.zeros(((nbytes + 3) // 4,), dtype=torch.float32, device="cuda")
    if pair:
        hip.check(lib.mccnn_ingest_u8_pair(hip.ptr(dev[0]), hip.ptr(dev[1]), H, W, C, hip.ptr(outs[0]), hip.ptr(outs[1]),
                                           hip.ptr(scratch), nbytes, hip.stream()), "mccnn_ingest_u8_pair")
    else:
        hip.check(lib.mccnn_ingest_u8(hip.ptr(dev[0]), H, W, C, hip.ptr(outs[0]), hip.ptr(scratch), nbytes, hip.stream()),
                  "mccnn_ingest_u8")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    differ = ih.bits(got) != ih.bits(want)
    assert not differ.any(), "%s: %d of %d patterns differ (first at %s: %r against %r)" % (
        what, int(differ.sum()), differ.size, np.argwhere(differ)[0], got[differ][0], want[differ][0])


@pytest.mark.parametrize("shape", ih.SHAPES, ids=lambda s: "%dx%d" % s)
def test_ingest_equals_numpy_bit_for_bit(shape):
    """out == (g - np.mean(g)) / np.std(g) as uint32 patterns for C = 1, 3, 4 and the three histograms: the single call
    and the pair call (two different images of the case)."""
    for hist in ih.HISTOGRAMS:
        for C in (1, 3, 4):
            a = ih.image_u8(shape, hist, C, seed=7)
            b = ih.image_u8(shape, hist, C, seed=8)
            wa, wb = ih.numpy_standardise(ih.gray_of(a)), ih.numpy_standardise(ih.gray_of(b))
            what = "%dx%d %s C=%d" % (shape + (hist, C))
            _same(_ingest_abi([a], False)[0], wa, what + " single")
            ga, gb = _ingest_abi([a, b], True)
            _same(ga, wa, what + " pair, left")
            _same(gb, wb, what + " pair, right")


def test_ingest_constant_image_gives_what_numpy_gives():
    for shape, value in (((40, 64), 77), ((97, 1031), 0), ((500, 750), 255), ((375, 1242), 131)):
        g8 = np.full(shape, value, np.uint8)
        _same(_ingest_abi([g8], False)[0], ih.numpy_standardise(g8), "constant %d %s" % (value, shape))
        rgb = np.repeat(g8[:, :, None], 3, axis=2)
        _same(_ingest_abi([rgb, rgb], True)[1], ih.numpy_standardise(ih.gray_of(rgb)), "constant rgb %d %s" % (value, shape))


@pytest.mark.parametrize("name", ["rgb", "rgba"])
def test_ingest_golden_colour_png(name):
    """The two colour PNGs pinned against libpng: bytes as PIL stores them -> the device's grey stage + standardisation
    equals NumPy's on util.read_gray's output and on the libpng grey fixture."""
    from PIL import Image
    import util
    path = os.path.join(GOLDEN_DIR, "png_color_%s.png" % name)
    im = Image.open(path)
    assert im.mode == name.upper()
    raw = np.asarray(im, dtype=np.uint8)
    assert raw.shape[2] == len(name)
    libpng_gray = np.load(os.path.join(GOLDEN_DIR, "png_gray_%s.npy" % name))
    assert np.array_equal(util.read_gray(path), libpng_gray)
    got = _ingest_abi([raw], False)[0]
    _same(got, ih.numpy_standardise(util.read_gray(path)), name)
    _same(got, ih.numpy_standardise(libpng_gray.astype(np.uint8)), name + " (libpng fixture)")


def test_host_wrappers():
    import torch
    import stereo_device as sd
    a, b = ih.image_u8((97, 1031), "uniform", 3, 1), ih.image_u8((97, 1031), "uniform", 3, 2)
    l, r = sd.ingest_u8_pair(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    _same(l.cpu().numpy(), ih.numpy_standardise(ih.gray_of(a)), "wrapper pair left")
    _same(r.cpu().numpy(), ih.numpy_standardise(ih.gray_of(b)), "wrapper pair right")
    g = ih.image_u8((8, 1029), "narrow_200_255", 1, 3)
    _same(sd.ingest_u8(torch.from_numpy(g).cuda()).cpu().numpy(), ih.numpy_standardise(g), "wrapper single")
    with pytest.raises(ValueError):
        sd.ingest_u8_pair(torch.from_numpy(a).cuda(), torch.from_numpy(g).cuda())


@pytest.mark.parametrize("H,W,D", [(40, 64, 16), (500, 750, 256)], ids=["40x64x16", "750x500x256"])
def test_match_from_bytes_equals_match_on_host_standardised_images(net_layers, H, W, D):
    """match_u8 and match_graph_u8 (three different pairs of one shape: capture, then two replays) return, bit for bit,
    what match() returns on the images standardised on the host as match.py does."""
    import torch
    import _hipabi as hip
    import stereo_device as sd
    import synthetic
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    matcher = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
    plain = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
    pairs = []
    for i in range(3):
        l8, r8, _ = synthetic.make_scene_u8(H, W, D, seed=300 + i)
        if i == 1:                                   # one of them as colour bytes
            l8 = np.ascontiguousarray(np.stack([l8, l8 // 2, 255 - l8], axis=2))
            r8 = np.ascontiguousarray(np.stack([r8, r8 // 2, 255 - r8], axis=2))
        pairs.append((l8, r8))
    for i, (l8, r8) in enumerate(pairs):
        host = [torch.from_numpy(ih.numpy_standardise(ih.gray_of(x))).cuda() for x in (l8, r8)]
        want = plain.match(host[0], host[1], D).cpu().numpy()
        dl, dr = torch.from_numpy(l8).cuda(), torch.from_numpy(r8).cuda()
        _same(matcher.match_u8(dl, dr, D).cpu().numpy(), want, "match_u8, pair %d" % i)
    grey = [p for p in pairs if p[0].ndim == 2] + [(ih.gray_of(pairs[1][0]), ih.gray_of(pairs[1][1]))]
    for i, (l8, r8) in enumerate(grey):
        host = [torch.from_numpy(ih.numpy_standardise(x)).cuda() for x in (l8, r8)]
        want = plain.match(host[0], host[1], D).cpu().numpy()
        got = matcher.match_graph_u8(torch.from_numpy(l8).cuda(), torch.from_numpy(r8).cuda(), D)
        _same(got.cpu().numpy(), want, "match_graph_u8, pair %d" % i)
    assert len(matcher._graphs) == 1                 # one capture, then replays
    l8, r8 = pairs[1]                                # pinned host bytes, another channel count: a graph of its own
    got = matcher.match_graph_u8(torch.from_numpy(l8).pin_memory(), torch.from_numpy(r8).pin_memory(), D)
    host = [torch.from_numpy(ih.numpy_standardise(ih.gray_of(x))).cuda() for x in (l8, r8)]
    _same(got.cpu().numpy(), plain.match(host[0], host[1], D).cpu().numpy(), "match_graph_u8 from pinned RGB bytes")
    assert len(matcher._graphs) == 2
