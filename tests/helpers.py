import contextlib

import numpy as np

_QNAN = np.uint32(0x7fc00000)


def _canonical_bits(a):
    """uint32 patterns of a float32 array with every NaN mapped to one pattern (sign and payload dropped): NumPy on the
    host and the GPU both return A quiet NaN for an invalid operation, but which payload / sign is not part of IEEE 754
    and differs between x86 (default NaN = negative quiet NaN) and gfx950 (positive)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = _QNAN
    return u


def bits_strict(a, b):
    """Bit-for-bit equality of two arrays.  float32: compared through their uint32 patterns, so +0.0 != -0.0; only NaN
    payloads are canonicalised (_canonical_bits)."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.array_equal(_canonical_bits(a), _canonical_bits(b)))
    return bool(np.array_equal(a, b))


def bits_equal(a, b):
    """The strict comparison (kept under the name the tests have always used; until round 6 it also let +0 == -0 pass)."""
    return bits_strict(a, b)


def bits_equal_up_to_zero_sign(a, b):
    """bits_strict() that lets +0.0 == -0.0 pass: only for the places listed in DESIGN.md section 2 where a sign of zero
    is known to differ from the reference and no consumer can see it."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        same = _canonical_bits(a) == _canonical_bits(b)
        same |= (a == b)
        return bool(same.all())
    return bool(np.array_equal(a, b))


def hp_of(g):
    return dict(zip([str(k) for k in g["hp_names"]], [float(v) for v in g["hp_values"]]))


def _describe(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s against %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
    if a.dtype == np.float32:
        ua, ub = _canonical_bits(a), _canonical_bits(b)
        differ = ua != ub
        zero_sign = differ & (a == b)
        with np.errstate(invalid="ignore"):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        mx = float(np.nanmax(d)) if np.isfinite(d).any() else float("nan")
        return "max abs diff %g, %d of %d patterns differ (%d of them only in the sign of a zero)" % (
            mx, int(differ.sum()), a.size, int(zero_sign.sum()))
    return "%d of %d differ" % (int((a != b).sum()), a.size)


def assert_bits_strict(a, b, what):
    assert bits_strict(a, b), "%s: not bit-identical (%s)" % (what, _describe(a, b))


def assert_bits(a, b, what):
    """Strict since round 6: uint32 patterns, signs of zeros included, NaN payloads canonicalised only."""
    assert_bits_strict(a, b, what)


@contextlib.contextmanager
def module_setting(module, name, value):
    """Sets a module-level switch (process_functional.CBCA_ORDER, ...) for a block and puts back whatever stood there,
    so that no test decides which kernel a later test's un-set call reaches."""
    previous = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, previous)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def stagewise(keep, L, R, D, o, hp=None, features=None):
    """Feeds every stage output a matcher handed out through `keep` to the CPU checker's next stage (`o`: the oracle
    module; `hp`: the matcher's hyper-parameters, default match.py's).  Returns {stage: max |gpu - cpu|} in stage order
    (0.0 = all bits equal; a zero of the other sign counts as the smallest subnormal).  features=(fl, fr): the cost
    volume is checked against the oracle's from these features too."""
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    tau, dist = a["cbca_intensity"], a["cbca_distance"]
    d = {}

    def diff(x, y):
        x = _host(x)
        if bits_strict(x, y):
            return 0.0
        m = float(np.nanmax(np.abs(x.astype(np.float64) - y))) if x.shape == np.shape(y) else float("inf")
        return m if m > 0.0 else float(np.spacing(np.float32(0)))     # a zero of the other sign: not 'all bits equal'

    cv = [_host(t) for t in keep["cv"]]
    if features is not None:
        ocv = o.compute_cost_volume(_host(features[0]), _host(features[1]), D)
        d["cost_volume"] = max(diff(cv[0], ocv[0]), diff(cv[1], ocv[1]))
    c1 = o.cost_volume_aggregation(L, R, cv[0], cv[1], tau, dist, a["cbca_num_iterations1"])
    d["cbca_x%d" % a["cbca_num_iterations1"]] = max(diff(keep["cbca1"][0], c1[0]), diff(keep["cbca1"][1], c1[1]))
    g1 = [_host(t) for t in keep["cbca1"]]
    s = o.SGM_average(g1[0].copy(), g1[1].copy(), L, R, a["sgm_P1"], a["sgm_P2"], a["sgm_Q1"], a["sgm_Q2"], a["sgm_D"],
                      a["sgm_V"])
    d["sgm"] = max(diff(keep["sgm"][0], s[0]), diff(keep["sgm"][1], s[1]))
    gs = [_host(t) for t in keep["sgm"]]
    n2 = a["cbca_num_iterations2"]
    c2 = o.cost_volume_aggregation(L, R, gs[0], gs[1], tau, dist, n2)
    d["cbca_x%d" % n2] = max(diff(keep["cbca2"][0], c2[0]), diff(keep["cbca2"][1], c2[1]))
    d["cbca_x%d_spacings_of_max_input" % n2] = d["cbca_x%d" % n2] / float(np.spacing(np.float32(np.abs(gs[0]).max())))
    g2 = [_host(t) for t in keep["cbca2"]]
    dl, dr = o.disparity_prediction(g2[0], g2[1])
    gdl, gdr = _host(keep["wta"][0]), _host(keep["wta"][1])
    d["wta_mismatches"] = int((gdl != dl).sum() + (gdr != dr).sum())
    di = o.interpolation(gdl, gdr, D)
    d["interpolation"] = diff(keep["interp"], di)
    ds = o.subpixel_enhance(_host(keep["interp"]), g2[0])
    d["subpixel"] = diff(keep["subpixel"], ds)
    dm = o.median_filter(_host(keep["subpixel"]), 5, 5)
    d["median"] = diff(keep["median"], dm)
    db = o.bilateral_filter(L, _host(keep["median"]), 5, 5, 0, a["blur_sigma"], a["blur_threshold"])
    d["bilateral"] = diff(keep["bilateral"], db)
    return d


def first_differing_stage(d):
    """The first stage of a stagewise() record whose output differs from the CPU checker's, or None."""
    return next((k for k, v in d.items() if v != 0 and not k.endswith("_spacings_of_max_input")), None)
