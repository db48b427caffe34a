"""The paper's SGM stage on the CPU: the four directional volumes each computed from the SAME input and averaged,

    L_r = semi_global_matching(copy of C, r, P1 (P1 / V for vertical r), P2, Q1, Q2, D, side)
    out = (((L_right + L_left) + L_up) + L_bottom) / 4.          float32, in that order

which is pf:210 / pf:232 evaluated on four independent arrays (the reference evaluates it on four aliases of one array,
because semi_global_matching returns its argument).  Built from oracle.semi_global_matching on copies and NumPy's float32
sum; the inputs are left as they are."""
import numpy as np

import oracle as o

DIRECTIONS = ((0, 1), (0, -1), (-1, 0), (1, 0))     # right, left, up, bottom (pf:194-208)
NAMES = ("right", "left", "up", "bottom")


def single_direction(volume, left_image, right_image, r, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V, choice):
    """L_r of `volume` [D,H,W] (a new array)."""
    v = np.ascontiguousarray(volume, dtype=np.float32).copy()
    p1 = sgm_P1 if r[0] == 0 else sgm_P1 / sgm_V
    o.semi_global_matching(left_image, right_image, v, r, p1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, choice)
    return v


def average4(parts):
    """(((a + b) + c) + d) / 4. in float32."""
    a, b, c, d = (np.asarray(p, dtype=np.float32) for p in parts)
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((a + b) + c) + d
        out = s / np.float32(4.)
    assert out.dtype == np.float32
    return out


def sgm_independent(volume, left_image, right_image, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V, choice):
    """The averaged volume of one side ("L" or "R")."""
    return average4([single_direction(volume, left_image, right_image, r, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V,
                                      choice) for r in DIRECTIONS])


def SGM_average_independent(left_cost_volume, right_cost_volume, left_image, right_image, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2,
                            sgm_D, sgm_V):
    """SGM_average's signature; returns new (left, right) arrays and modifies nothing."""
    return (sgm_independent(left_cost_volume, left_image, right_image, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V, "L"),
            sgm_independent(right_cost_volume, left_image, right_image, sgm_P1, sgm_P2, sgm_Q1, sgm_Q2, sgm_D, sgm_V, "R"))


def match_from_cost_volumes(left_image, right_image, cv_l, cv_r, ndisp, independent, hp=None, return_all=False):
    """The timed region behind the cost volume (oracle.match_from_features' chain) with either SGM stage."""
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    sgm = [a[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]
    c1 = o.cost_volume_aggregation(left_image, right_image, cv_l, cv_r, a["cbca_intensity"], a["cbca_distance"],
                                   a["cbca_num_iterations1"])
    if independent:
        s = SGM_average_independent(c1[0], c1[1], left_image, right_image, *sgm)
    else:
        s = o.SGM_average(c1[0].copy(), c1[1].copy(), left_image, right_image, *sgm)
    c2 = o.cost_volume_aggregation(left_image, right_image, s[0], s[1], a["cbca_intensity"], a["cbca_distance"],
                                   a["cbca_num_iterations2"])
    dl, dr = o.disparity_prediction(c2[0], c2[1])
    di = o.interpolation(dl, dr, ndisp)
    ds = o.subpixel_enhance(di, c2[0])
    dm = o.median_filter(ds, 5, 5)
    db = o.bilateral_filter(left_image, dm, 5, 5, 0, a["blur_sigma"], a["blur_threshold"])
    if return_all:
        return db, dict(cbca1=c1, sgm=s, cbca2=c2, wta=(dl, dr), interp=di, subpixel=ds, median=dm, bilateral=db)
    return db
