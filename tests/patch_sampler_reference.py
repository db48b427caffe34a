"""A literal NumPy restatement of mccnn_sample_patches (include/mccnn.h, csrc/sample.hip): per output pixel, every
operation a float32 operation of its own, in the order the header states.  Slow on purpose; the tests compare the kernel
with it as uint32 patterns."""
import numpy as np

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)


def _tap(img, yf, xf):
    H, W = img.shape
    if ZERO <= yf <= f32(H - 1) and ZERO <= xf <= f32(W - 1):       # compared as floats, before any conversion
        return img[int(yf), int(xf)]
    return ZERO


def _row(img, yy, x0, fx):
    a = _tap(img, yy, x0)
    if fx == ZERO:
        return a                                                     # the second tap is not read
    b = _tap(img, yy, f32(x0 + ONE))
    wa = f32(ONE - fx)
    return f32(f32(a * wa) + f32(b * fx))


def sample_pixel(img, rec, ps, i, j):
    c = f32((ps - 1) // 2)
    u, v = f32(f32(j) - c), f32(f32(i) - c)
    m = [f32(t) for t in rec["m"]]
    cx, cy, gain, bias = f32(rec["cx"]), f32(rec["cy"]), f32(rec["gain"]), f32(rec["bias"])
    x = f32(cx + f32(f32(m[0] * u) + f32(m[1] * v)))
    y = f32(cy + f32(f32(m[2] * u) + f32(m[3] * v)))
    x0, y0 = f32(np.floor(x)), f32(np.floor(y))
    fx, fy = f32(x - x0), f32(y - y0)
    val = _row(img, y0, x0, fx)
    if fy != ZERO:
        below = _row(img, f32(y0 + ONE), x0, fx)
        wa = f32(ONE - fy)
        val = f32(f32(val * wa) + f32(below * fy))
    if not (gain == ONE and bias == ZERO):
        val = f32(f32(val * gain) + bias)
    return val


def sample_patches(images, records, ps):
    """images: list of [H, W] float32 arrays (the pool, image by image); records: array of datagenerator.SAMPLE_DTYPE.
    Returns [N, ps, ps] float32."""
    images = [np.ascontiguousarray(im, dtype=np.float32) for im in images]
    out = np.zeros((len(records), ps, ps), dtype=np.float32)
    with np.errstate(all="ignore"):
        for n, rec in enumerate(records):
            img = images[int(rec["image"])]
            for i in range(ps):
                for j in range(ps):
                    out[n, i, j] = sample_pixel(img, rec, ps, i, j)
    return out


def _taps(pool, off, H, W, yf, xf):
    """tap() on arrays: pool flat float32, off / H / W per record broadcast over the patch."""
    ok = (yf >= ZERO) & (yf <= (H - 1).astype(np.float32)) & (xf >= ZERO) & (xf <= (W - 1).astype(np.float32))
    yi = np.where(ok, yf, ZERO).astype(np.int64)
    xi = np.where(ok, xf, ZERO).astype(np.int64)
    return np.where(ok, pool[np.where(ok, off + yi * W + xi, 0)], ZERO)


def sample_patches_arrays(images, records, ps):
    """The same arithmetic on whole arrays (every NumPy float32 array operation rounds on its own, like the scalar
    ones): for the shapes at which the per-pixel loop takes too long.  tests/test_patch_sampler_cpu.py pins it to
    sample_patches bit for bit."""
    images = [np.ascontiguousarray(im, dtype=np.float32) for im in images]
    pool = np.concatenate([im.ravel() for im in images])
    starts = np.cumsum([0] + [im.size for im in images[:-1]]).astype(np.int64)
    k = records["image"].astype(np.int64)
    off = starts[k][:, None, None]
    H = np.array([im.shape[0] for im in images], dtype=np.int64)[k][:, None, None]
    W = np.array([im.shape[1] for im in images], dtype=np.int64)[k][:, None, None]
    c = f32((ps - 1) // 2)
    u = (np.arange(ps, dtype=np.float32) - c)[None, None, :]
    v = (np.arange(ps, dtype=np.float32) - c)[None, :, None]
    m = records["m"].astype(np.float32)[:, :, None, None]
    cx, cy = (records[n].astype(np.float32)[:, None, None] for n in ("cx", "cy"))
    gain, bias = (records[n].astype(np.float32)[:, None, None] for n in ("gain", "bias"))
    with np.errstate(all="ignore"):
        x = cx + ((m[:, 0] * u) + (m[:, 1] * v))
        y = cy + ((m[:, 2] * u) + (m[:, 3] * v))
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0

        def row(yy):
            a = _taps(pool, off, H, W, yy, x0)
            b = _taps(pool, off, H, W, yy, x0 + ONE)
            return np.where(fx == ZERO, a, (a * (ONE - fx)) + (b * fx))

        top = row(y0)
        val = np.where(fy == ZERO, top, (top * (ONE - fy)) + (row(y0 + ONE) * fy))
        out = np.where((gain == ONE) & (bias == ZERO), val, (val * gain) + bias)
    assert out.dtype == np.float32 and x.dtype == np.float32
    return np.ascontiguousarray(out)


def mixed_records(shapes, N, ps, seed):
    """N records over images of the given (H, W) shapes that mix what the kernel must get right: identity records,
    fractional centres, centres outside the image by up to ps, centres at +-1e30, rotations up to 28 degrees with scales
    down to 0.64 and shear 0.4, and gains and biases away from (1, 0)."""
    from datagenerator import SAMPLE_DTYPE, _inverse_2x2, augment_matrix
    rng = np.random.default_rng(seed)
    rec = np.zeros(N, dtype=SAMPLE_DTYPE)
    rec["image"] = rng.integers(0, len(shapes), size=N)
    H = np.array([s[0] for s in shapes])[rec["image"]]
    W = np.array([s[1] for s in shapes])[rec["image"]]
    kind = (np.arange(N) + rng.integers(0, 7)) % 7
    cy = rng.integers(0, H).astype(np.float64)
    cx = rng.integers(0, W).astype(np.float64)
    frac = kind >= 1
    cy = np.where(frac, rng.uniform(-1.0, H, size=N), cy)
    cx = np.where(frac, rng.uniform(-1.0, W, size=N), cx)
    outside = kind == 2
    cy = np.where(outside, np.where(rng.random(N) < 0.5, -rng.uniform(0, ps, size=N), H - 1 + rng.uniform(0, ps, size=N)), cy)
    cx = np.where(outside, np.where(rng.random(N) < 0.5, -rng.uniform(0, ps, size=N), W - 1 + rng.uniform(0, ps, size=N)), cx)
    far = kind == 3
    cy = np.where(far, np.where(rng.random(N) < 0.5, -1e30, 1e30), cy)
    cx = np.where(far & (rng.random(N) < 0.7), np.where(rng.random(N) < 0.5, -1e30, 1e30), cx)
    warped = kind >= 4
    s = rng.uniform(0.8, 1.0, size=N)
    A = augment_matrix(s * rng.uniform(0.8, 1.0, size=N), s, rng.uniform(-0.4, 0.4, size=N),
                       rng.uniform(-28, 28, size=N) * np.pi / 180)
    m = np.where(warped[:, None], _inverse_2x2(A).reshape(N, 4), np.array([1.0, 0, 0, 1]))
    toned = (kind == 5) | (kind == 6)
    rec["cy"], rec["cx"], rec["m"] = cy, cx, m
    rec["gain"] = np.where(toned, rng.uniform(1 / 1.3, 1.3, size=N), 1.0)
    rec["bias"] = np.where(kind == 6, rng.uniform(-1.3, 1.3, size=N), 0.0)
    return rec


def planted_images(shapes, seed):
    """Standard-normal images of the given shapes with -0.0 planted at two corners and in the interior."""
    rng = np.random.default_rng(seed)
    images = []
    for H, W in shapes:
        img = rng.standard_normal((H, W)).astype(np.float32)
        img[0, 0] = img[H - 1, W - 1] = img[H // 2, W // 2] = img[H // 3, W // 4] = -0.0
        images.append(img)
    return images
