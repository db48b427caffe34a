"""GPU: MCCNN_CBCA_SEPARABLE (mccnn_cbca_iter / mccnn_cbca_iter_pair, csrc/cross_cbca.hip) against the float64 region
mean, summed directly from the arms (tests/fast_kernels_reference.py: region_mean64) - something that does not share
the float32 summation order the other tests compare with.

Distance <= 14, cbca_stream_kernel (float64 prefix sums): one iteration, every voxel,
    |got - mean64| <= 0.5 ulp32(mean64) + 2^-34 max|in|
(the correctly rounded mean plus what the float64 prefix differences can lose; the CPU test of the references checks
that the kernel's stated algorithm stays inside it and that a float32 column prefix does not).  The shapes walk the
launch geometry: 256-column strips, row chunks of at least 64 rows, the 32-row ring, batches of three rows, two planes
per workgroup, whole rounds plus a chunked remainder, two jobs per launch.  Containment: the planes lie inside larger
allocations (NaN around the input, a sentinel around the output) and the result has the bits of the stand-alone run.

Distance 15 .. 32, cbca_iter_kernel<31, 16, false> (sequential float32 sums of the arms): NOT correctly rounded; the
textbook bound (n_h + n_v + 2) 2^-24 (sum over the region of |v|) / n holds per voxel.

The worst error per shape and volume goes to parity_cbca_separable.json in the directory MCCNN_RECORD_DIR names
(profiles/parity_cbca_separable.json is a copy)."""
import json
import os

import numpy as np
import pytest
import torch

import fast_kernels_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


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
        path = os.path.join(out, "parity_cbca_separable.json")
        old = {}
        if os.path.isfile(path):
            with open(path) as f:
                old = json.load(f)
        old.update(record)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


def planes_of(D):
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count + 2 if D is None else D


_cases = {}


def case(sd, H, W, D, L, which=0):
    """The image, its support plane (device), arms (host) and the three volumes of one shape, built once.  `which`
    selects a second, different image and set of volumes for the right-hand job of a pair launch."""
    key = (H, W, D, L, which)
    if key not in _cases:
        seed = R.cbca_case_seed(H, W, L) + 7919 * which
        sup = sd.cross_arms(dev(R.cbca_image(H, W, seed)), R.CBCA_TAU, L)
        count = sd.support_count(sup).cpu().numpy()
        # the inputs must not quietly become trivial: arms at the limit and textured pixels whose region is themselves
        assert count.max() > R.nontrivial_region_floor(H, W, L), "largest region %d" % count.max()
        assert (count == 1).any(), "no region of size 1"
        arms = sd.support_arms(sup).cpu().numpy()
        assert np.array_equal(R.region_count(arms), count)
        vols = R.cbca_volumes(D, H, W, seed)
        for v in vols.values():
            v.setflags(write=False)
        _cases[key] = (sup, arms, vols)
    return _cases[key]


def run_single(sd, vol, sup, L):
    import _hipabi as hip
    v = dev(vol)
    out = torch.full_like(v, SENTINEL)
    got, _ = sd.cbca(v, out, sup, 1, L, hip.MCCNN_CBCA_SEPARABLE)
    assert got is out
    return got


def worst_in_ulps(got, mean):
    return float((np.abs(got.astype(np.float64) - mean) / R.ulp32(mean)).max())


@pytest.mark.parametrize("H,W,D", R.CBCA_STREAM_SHAPES, ids=["%dx%dx%s" % (h, w, d or "2CUs+2") for h, w, d in R.CBCA_STREAM_SHAPES])
def test_stream_kernel_returns_the_correctly_rounded_region_mean(sd, H, W, D):
    import _hipabi as hip
    L, D = 14, planes_of(D)
    jobs = [case(sd, H, W, D, L, which) for which in (0, 1)]
    record = {}
    for name in R.CBCA_VOLUMES:
        single = []
        for which, (sup, arms, vols) in enumerate(jobs):
            got = run_single(sd, vols[name], sup, L)
            single.append(got)
            if which:
                continue            # the second job is there for the pair launch; one float64 reference per volume
            mean = R.region_mean64(vols[name], arms)
            tolerance = R.separable_tolerance(mean, np.abs(vols[name]).max())
            g = got.cpu().numpy()
            err = np.abs(g.astype(np.float64) - mean)
            record[name] = {"worst_ulps": worst_in_ulps(g, mean), "worst_of_tolerance": float((err / tolerance).max())}
            print("%dx%dx%d %s: worst %.4f ulp, %.4f of the tolerance" % (H, W, D, name, record[name]["worst_ulps"],
                                                                          record[name]["worst_of_tolerance"]))
            bad = err > tolerance
            assert not bad.any(), "%s: %d voxels beyond 0.5 ulp + 2^-34 max|in|, the worst by %g ulp at %s" % (
                name, int(bad.sum()), record[name]["worst_ulps"], np.unravel_index(np.argmax(err / tolerance), err.shape))
        # both jobs in one launch: each equals its single launch bit for bit
        (sl, al, _), (sr, ar, _) = jobs
        vl, vr = dev(jobs[0][2][name]), dev(jobs[1][2][name])
        (pl, _), (pr, _) = sd.cbca_pair(vl, torch.full_like(vl, SENTINEL), sl, vr, torch.full_like(vr, SENTINEL), sr, 1, L,
                                        hip.MCCNN_CBCA_SEPARABLE)
        assert torch.equal(pl.view(torch.int32), single[0].view(torch.int32)), "%s: left job of the pair launch" % name
        assert torch.equal(pr.view(torch.int32), single[1].view(torch.int32)), "%s: right job of the pair launch" % name
    record_measured({"L14 %dx%dx%d" % (H, W, D): record})


@pytest.mark.parametrize("H,W,D", [(14, 257, 3), (33, 300, 5), (130, 40, 3)])
def test_stream_kernel_stays_inside_its_planes(sd, H, W, D):
    """`in` and `out` inside larger allocations: NaN in front of and behind the input (a read outside the volume would
    poison a row's prefix sums), a sentinel around the output.  The kernel addresses every plane through a buffer
    descriptor of its own; the columns left of the image, which read the end of the previous row, and the columns right
    of it never reach outside the plane."""
    import _hipabi as hip
    L = 14
    sup, arms, vols = case(sd, H, W, D, L)
    for name in R.CBCA_VOLUMES:
        alone = run_single(sd, vols[name], sup, L)
        n, margin = D * H * W, 4 * W + 64
        big_in = torch.full((n + 2 * margin,), float("nan"), device="cuda")
        big_out = torch.full((n + 2 * margin,), SENTINEL, device="cuda")
        vin, vout = big_in[margin:margin + n].view(D, H, W), big_out[margin:margin + n].view(D, H, W)
        vin.copy_(dev(vols[name]))
        sd.cbca(vin, vout, sup, 1, L, hip.MCCNN_CBCA_SEPARABLE)
        assert torch.equal(vout.view(torch.int32), alone.view(torch.int32)), "%s: not the bits of the stand-alone run" % name
        assert bool((big_out[:margin] == SENTINEL).all()) and bool((big_out[margin + n:] == SENTINEL).all()), \
            "%s: a store outside the volume" % name
        assert bool(torch.isnan(big_in[:margin]).all()) and bool(torch.isnan(big_in[margin + n:]).all())


@pytest.mark.parametrize("L,shape", R.CBCA_TILE_CASES, ids=["L%d-%dx%dx%d" % ((L,) + s) for L, s in R.CBCA_TILE_CASES])
def test_long_arm_separable_is_a_float32_sum_with_the_textbook_bound(sd, L, shape):
    """Distances 15 .. 32 take cbca_iter_kernel<31, 16, false>: horizontal and vertical arm sums in plain float32, up to
    63 + 63 sequential additions.  Not correctly rounded (include/mccnn.h says so); what holds per voxel is
    |got - mean64| <= (n_h + n_v + 2) 2^-24 (sum over the region of |v|) / n."""
    H, W, D = shape
    sup, arms, vols = case(sd, H, W, D, L)
    assert int(arms.max()) > 13, "no arm beyond what the streaming kernel serves"
    record = {}
    for name in R.CBCA_VOLUMES:
        got = run_single(sd, vols[name], sup, L).cpu().numpy()
        mean = R.region_mean64(vols[name], arms)
        bound = R.tile_kernel_bound(vols[name], arms)
        err = np.abs(got.astype(np.float64) - mean)
        record[name] = {"worst_ulps": worst_in_ulps(got, mean), "worst_of_bound": float((err / bound).max())}
        print("L=%d %dx%dx%d %s: worst %.3f ulp, %.4f of the bound" % (L, H, W, D, name, record[name]["worst_ulps"],
                                                                      record[name]["worst_of_bound"]))
        assert (err <= bound).all(), "%s: %d voxels beyond the sequential-sum bound" % (name, int((err > bound).sum()))
    record_measured({"L%d %dx%dx%d" % (L, H, W, D): record})
