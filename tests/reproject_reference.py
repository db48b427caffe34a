"""The metric outputs of include/mccnn.h restated in NumPy, literally: float32 scalars rounded once from float64, one
np.float32 operation per step in the stated order, np.flatnonzero for the order of the cloud.  Shared by the CPU and GPU
tests of the depth plane and the point cloud; never imported by the product."""
import numpy as np

INF = np.float32(np.inf)
f32 = np.float32


def scalars(calib):
    """(fx, fy, cx, cy, fb, doffs): each rounded once; fb from the float64 product fx * baseline."""
    fx, fy, cx, cy, baseline, doffs = (float(v) for v in calib)
    return f32(fx), f32(fy), f32(cx), f32(cy), f32(fx * baseline), f32(doffs)


def depth(disp, calib):
    """Z = fb / (d + doffs) where d is finite and the sum positive, +inf elsewhere."""
    disp = np.ascontiguousarray(disp, dtype=np.float32)
    _fx, _fy, _cx, _cy, fb, doffs = scalars(calib)
    with np.errstate(all="ignore"):
        den = disp + doffs                       # one float32 add
        has = np.isfinite(disp) & (den > f32(0))
        z = np.full(disp.shape, INF, dtype=np.float32)
        z[has] = fb / den[has]                   # a correctly rounded float32 division
    assert z.dtype == np.float32
    return z


def kept(z, max_depth=np.inf):
    return np.isfinite(z) & (z <= f32(max_depth))


def points(disp, calib, max_depth=np.inf):
    """[n,4] float32 records (X, Y, Z, the bits of the uint32 h * W + w) of the kept pixels in raster order."""
    fx, fy, cx, cy, _fb, _doffs = scalars(calib)
    z = depth(disp, calib)
    H, W = z.shape
    index = np.flatnonzero(kept(z, max_depth)).astype(np.uint32)
    h, w = index // np.uint32(W), index % np.uint32(W)
    zk = z.reshape(-1)[index]
    with np.errstate(all="ignore"):
        x = ((w.astype(np.float32) - cx) * zk) / fx          # sub, mul, div
        y = ((h.astype(np.float32) - cy) * zk) / fy
    assert x.dtype == np.float32 and y.dtype == np.float32 and zk.dtype == np.float32
    out = np.empty((index.size, 4), dtype=np.uint32)         # words, so that no float copy touches the index
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = bits(x), bits(y), bits(zk), index
    return out.view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ramp(H, W, lo=0.5, hi=60.0):
    """A smooth ramp of disparities with a little structure: no two rows equal."""
    h, w = np.mgrid[0:H, 0:W]
    return (lo + (hi - lo) * (w + 0.37 * h) / max(1.0, W + 0.37 * H)).astype(np.float32)
