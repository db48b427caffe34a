"""GPU: cost volumes of 4 GiB and more (full-resolution Middlebury: 2880 x 1988 x 256 is 5.9 GB).  The oracle is too
slow at this size, so exactness is carried over from smaller runs that the oracle pins: the same scanlines computed on
a crop of the volume below 4 GiB (the existing kernels) must come out bit for bit the same as on the whole volume (the
vertical passes rebase their buffer descriptor there).  Then whole pairs past 4 GiB: the default pixel-major
StereoMatcher against its plane-major twin, and process_functional.SGM_average against the pixel-major route.
Every test stays under about 40 GB of device memory."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GIB4 = 1 << 32
SGM_HP = (2.3, 55.9, 4, 8, 0.08)


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _volume(H, W, Dp, seed):
    """A pixel-major volume of random costs in [-2, 2) with about 1 % +inf, generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.rand((H, W, Dp), device="cuda", generator=g)
    inf = torch.rand((H, W, Dp), device="cuda", generator=g) < 0.01
    v.mul_(4).sub_(2).masked_fill_(inf, float("inf"))
    del inf
    v[:, :, 0] = torch.where(torch.isinf(v[:, :, 0]), torch.ones_like(v[:, :, 0]), v[:, :, 0])
    return v


def _images(H, W, seed):
    """Images whose steps straddle the 0.08 edge threshold, so that both penalty classes occur."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((H, W), device="cuda", generator=g) * 0.07, torch.randn((H, W), device="cuda", generator=g) * 0.07)


def _pass(sd, l, r, vol, side, D, r_):
    p1, p2, q1, q2, thr = (sd._f32(x) for x in SGM_HP)
    H, W = l.shape
    sd.sgm_pass_hwd(l, r, [vol], [side], D, r_, p1, p2, q1, q2, thr, sd.sgm_scratch(H, W, D, l.device))


@pytest.mark.parametrize("H,W,D,cut", [(1100, 1000, 1024, 100), (2100, 2100, 256, 200)], ids=["d1024", "d256"])
def test_sgm_passes_past_4gib_equal_their_crops(sd, H, W, D, cut):
    """Each single pass, both directions of each axis: horizontal passes on a row slab, vertical passes of the left
    volume (x = w - d) on the columns [0, W - cut), of the right volume (x = w + d) on [cut, W) - each crop sees the
    same flag lookups and skip tests as the whole image and stays below 4 GiB."""
    import _hipabi as hip
    Dp = sd.hwd_pitch(D)
    assert H * W * Dp * 4 >= GIB4
    assert H * (W - cut) * Dp * 4 < GIB4 and (H - cut) * W * Dp * 4 < GIB4
    base = _volume(H, W, Dp, seed=D)
    l, r = _images(H, W, seed=D + 1)
    cases = [((0, 1), hip.MCCNN_SIDE_LEFT, (slice(0, H - cut), slice(None))),
             ((0, -1), hip.MCCNN_SIDE_RIGHT, (slice(cut, H), slice(None))),
             ((1, 0), hip.MCCNN_SIDE_LEFT, (slice(None), slice(0, W - cut))),
             ((-1, 0), hip.MCCNN_SIDE_LEFT, (slice(None), slice(0, W - cut))),
             ((1, 0), hip.MCCNN_SIDE_RIGHT, (slice(None), slice(cut, W))),
             ((-1, 0), hip.MCCNN_SIDE_RIGHT, (slice(None), slice(cut, W)))]
    for r_, side, (rows, cols) in cases:
        whole = base.clone()
        _pass(sd, l, r, whole, side, D, r_)
        got = whole[rows, cols]
        assert not _same_bits(got[:, :, :D], base[rows, cols][:, :, :D]), "the pass changed nothing"
        crop = base[rows, cols].clone(memory_format=torch.contiguous_format)   # (base itself stays untouched)
        _pass(sd, l[rows, cols].contiguous(), r[rows, cols].contiguous(), crop, side, D, r_)
        assert _same_bits(got[:, :, :D], crop[:, :, :D]), "D=%d r=%s side %d: whole volume differs from its crop" % (
            D, r_, side)
        del whole, crop, got
        torch.cuda.empty_cache()


def test_sgm_average_past_4gib_plane_major_equals_pixel_major(sd):
    """process_functional.SGM_average at D <= 256 on plane-major volumes past 4 GiB (its first pass cannot gather the
    volume through one descriptor and runs as layout change + pass) equals the pixel-major route: layout change, then
    the four passes of sgm_average_hwd."""
    import process_functional as pf
    H, W, D = 2048, 2100, 256
    assert D * H * W * 4 >= GIB4
    g = torch.Generator(device="cuda").manual_seed(9)
    vl = torch.rand((D, H, W), device="cuda", generator=g).mul_(4).sub_(2)
    vr = torch.rand((D, H, W), device="cuda", generator=g).mul_(4).sub_(2)
    l, r = _images(H, W, seed=10)
    ha, hb = sd.dhw_to_hwd(vl), sd.dhw_to_hwd(vr)
    sd.sgm_average_hwd(l, r, [ha, hb], [0, 1], D, *SGM_HP, 1.5, sd.sgm_scratch(H, W, D, l.device))
    ol, orr = pf.SGM_average(vl, vr, l, r, *SGM_HP, 1.5)
    del ol, orr
    torch.cuda.empty_cache()
    for name, got, hw in (("left", vl, ha), ("right", vr, hb)):
        want = sd.hwd_to_dhw(hw, D)
        assert _same_bits(got, want), "SGM_average past 4 GiB (%s) differs from the pixel-major route" % name
        del want


def test_pair_past_4gib_pixel_major_equals_plane_major(net_layers, sd):
    """A whole pair whose volumes exceed 4 GiB (2100 x 2048 x 256: 4.4 GB each): the default StereoMatcher (pixel-major
    from the cost volume on) against its layout="plane_major" twin, which runs the plane-major kernels and the layout
    changes around SGM - final maps and both WTA maps bit for bit.  The matchers run one after the other, so that only
    one workspace is resident."""
    import synthetic
    from model import NET
    H, W, D = 2048, 2100, 256
    assert H * W * sd.hwd_pitch(D) * 4 >= GIB4
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=12)
    l, r = torch.from_numpy(L[:, :, 0].copy()).cuda(), torch.from_numpy(R[:, :, 0].copy()).cuda()
    res = []
    for layout in ("auto", "plane_major"):
        m = sd.StereoMatcher(net, layout=layout)
        assert m.pixel_major() == (layout == "auto")
        out = m.match(l, r, D)
        maps = m._ws[(H, W, D)]["maps"]
        res.append((out.cpu(), maps[0].cpu(), maps[1].cpu()))
        del m, out, maps
        torch.cuda.empty_cache()
    for name, a, b in zip(("final map", "left WTA", "right WTA"), res[0], res[1]):
        assert _same_bits(a, b), "%s: pixel-major and plane-major differ past 4 GiB" % name
