"""GPU: the store paths of cost_volume_exact_pairs_kernel (csrc/cost_volume.hip) - full quads as one 16-byte store,
ragged quads float by float, in both volumes - through mccnn_cost_volume_hwd(MCCNN_CV_EXACT) and its border fill.

Every shape is compared, as uint32 patterns, with the CPU oracle and with the plane-major kernel's volumes moved to
pixel-major (mccnn_cost_volume + mccnn_dhw_to_hwd); the output buffers start out holding a sentinel, and the Dp - D pad
entries of every pixel must still hold it afterwards.

The reference defines the cost volume for D <= W - 2 only (its right-volume border recurrence reads columns left of 0
beyond that), and both the oracle and the C ABI refuse anything else.  Three of the shapes this file was asked to cover -
(2, 130, 130), (2, 100, 256) and (2, 50, 64) - lie outside that envelope.  They are kept: for them the test pins what
the entry point does (MCCNN_E_UNSUPPORTED, the buffers untouched), and the nearest shapes inside the envelope that reach
what they were chosen for run the full comparison instead: (2, 132, 130) has the last tile with nd = 2 and Dp > D,
(2, 258, 256) and (2, 66, 64) have D = W - 2, the most w < d entries a shape can have."""
import numpy as np
import pytest
import torch

from helpers import assert_bits_strict

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)

# (H, W, D): what each one reaches first
SHAPES = [
    (2, 130, 64),     # a fully interior tile, the diagonal tile and a right-edge tile
    (2, 130, 130),    # (outside the envelope) a last tile with nd = 2 and Dp > D
    (2, 132, 130),    # ... its neighbour inside the envelope
    (2, 260, 256),    # four tiles per workgroup, ring wrap
    (1, 750, 256),    # the benchmark's width: last tile 57 wide
    (2, 100, 256),    # (outside the envelope) W < D
    (2, 50, 64),      # (outside the envelope) W < D
    (2, 258, 256),    # D = W - 2
    (2, 66, 64),      # D = W - 2, one disparity tile
    (3, 63, 5),       # tile boundaries at 62 / 63 / 64, D not a multiple of 4
    (2, 64, 4),
    (2, 65, 61),
]


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


def _features(H, W, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H, W, 64)).astype(np.float32), rng.standard_normal((H, W, 64)).astype(np.float32))


_reference = {}


def reference(key, fl, fr, D):
    """The CPU oracle's volumes as [H, W, D], computed once per case and handed out read-only."""
    if key not in _reference:
        import oracle as o
        with np.errstate(all="ignore"):
            l, r = o.compute_cost_volume(fl, fr, D)
        out = tuple(np.ascontiguousarray(v.transpose(1, 2, 0)) for v in (l, r))
        for v in out:
            v.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_hwd(sd, fl, fr, D):
    """mccnn_cost_volume_hwd into sentinel-filled buffers -> two host arrays [H, W, Dp]."""
    H, W, _ = fl.shape
    Dp = sd.hwd_pitch(D)
    out = tuple(torch.full((H, W, Dp), float(SENTINEL), device="cuda") for _ in range(2))
    sd.cost_volume_hwd(fl, fr, D, out=out)
    return tuple(t.cpu().numpy() for t in out)


def check_against_everything(sd, key, fl_np, fr_np, D):
    fl, fr = dev(fl_np), dev(fr_np)
    got = run_hwd(sd, fl, fr, D)
    want = reference(key, fl_np, fr_np, D)
    planes = sd.cost_volume(fl, fr, D)
    for side, g, w, p in zip(("left", "right"), got, want, planes):
        assert_bits_strict(g[:, :, :D], w, "%s volume against the oracle" % side)
        moved = sd.dhw_to_hwd(p).cpu().numpy()
        assert_bits_strict(g[:, :, :D], moved[:, :, :D], "%s volume against mccnn_cost_volume + mccnn_dhw_to_hwd" % side)
        pad = g[:, :, D:]
        assert pad.size == 0 or bool((pad.view(np.uint32) == SENTINEL.view(np.uint32)).all()), \
            "%s volume: a pad entry (d >= D) was written" % side
    return got


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_store_paths_against_oracle_and_plane_major(sd, H, W, D):
    fl_np, fr_np = _features(H, W, seed=H * 100000 + W * 1000 + D)
    if D > W - 2:
        import _hipabi as hip
        fl, fr = dev(fl_np), dev(fr_np)
        Dp = sd.hwd_pitch(D)
        out = tuple(torch.full((H, W, Dp), float(SENTINEL), device="cuda") for _ in range(2))
        rc = hip.load().mccnn_cost_volume_hwd(hip.ptr(fl), hip.ptr(fr), H, W, 64, D, hip.ptr(out[0]), hip.ptr(out[1]),
                                              hip.MCCNN_CV_EXACT, hip.stream())
        assert rc == hip.MCCNN_E_UNSUPPORTED
        torch.cuda.synchronize()
        for t in out:
            assert bool((t == float(SENTINEL)).all()), "a refused call wrote to its output"
        import oracle as o
        with pytest.raises(ValueError):
            o.compute_cost_volume(fl_np, fr_np, D)
        return
    check_against_everything(sd, (H, W, D), fl_np, fr_np, D)


def _special_features(H, W):
    """One non-zero channel, so that a score is minus ONE exact product and special values land where they are put:
    every left pixel x right pixel pair of a row meets, so every kind of score occurs in interior quads (w >= d + 3,
    away from the tile edges) of all three tiles."""
    rng = np.random.default_rng(7)
    mags = np.array([0.0, -0.0, 1e-22, 1e-20, 3e-20, 1.0, -1.0, 0.75, 1e18, -1.8e19, 2.5e19, np.inf, -np.inf, np.nan],
                    np.float32)
    out = []
    for _ in range(2):
        f = np.zeros((H, W, 64), np.float32)
        m = rng.standard_normal((H, W)).astype(np.float32)
        hit = rng.random((H, W)) < 0.3
        m[hit] = mags[rng.integers(0, mags.size, int(hit.sum()))]
        f[:, :, 0] = m
        out.append(f)
    return out


def test_special_values_in_interior_quads(sd):
    H, W, D = 2, 130, 64
    fl_np, fr_np = _special_features(H, W)
    got = check_against_everything(sd, "special", fl_np, fr_np, D)
    # the scores themselves (w >= d + 3: quads no edge touches) hold every kind of value
    left = reference("special", fl_np, fr_np, D)[0]
    w, d = np.meshgrid(np.arange(W), np.arange(D), indexing="ij")
    interior = np.broadcast_to((w >= d + 3) & (w < W - 3), left.shape)
    v = left[interior]
    assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any()
    assert ((v == 0) & np.signbit(v)).any(), "no -0.0 among the interior scores"
    tiny = np.abs(v[np.isfinite(v) & (v != 0)])
    assert (tiny < 1.1e-38).any(), "no subnormal among the interior scores"
    assert np.isnan(got[0][:, :, :D][interior]).any()


def test_two_calls_are_bit_identical(sd):
    H, W, D = 2, 260, 256
    fl_np, fr_np = _features(H, W, seed=11)
    fl, fr = dev(fl_np), dev(fr_np)
    a = run_hwd(sd, fl, fr, D)
    b = run_hwd(sd, fl, fr, D)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
