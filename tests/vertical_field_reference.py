"""A field of row offsets (include/mccnn.h: mccnn_vertical_field_select, mccnn_cost_volume_field_hwd), restated in NumPy
on tests/vertical_offset_reference.py.

Grid: gh x gw cells; row band of image row h = h * gh // H, column band of column x = (x // 64) * gw // ceil(W / 64).

    totals[a][b][k + R] = the votes for k of the profiled rows h_i in row band a and the blocks in column band b
    field[a][b]         = offset_select's winner of the cell's totals; a cell without a vote takes the global winner

    F(h, x)    = clip(field[row band of h][column band of min(x, W - 1)], -8, 8)
    S_L(d,h,w) = offset_scores' S_L with k0 = F(h, w)
    S_R(d,h,w) = offset_scores' S_R with k0 = F(h, w + d)

then vertical_reference.fill_and_negate."""
import numpy as np

import vertical_offset_reference as vo
import vertical_reference as vr

FIELD_MAX = 8


def row_bands(H, gh):
    return np.arange(int(H)) * int(gh) // int(H)


def column_bands(W, gw):
    nb = (int(W) + 63) // 64
    return (np.arange(int(W)) // 64) * int(gw) // nb


def clamped(field):
    return np.clip(np.asarray(field, np.int64), -vo.OFFSET_MAX, vo.OFFSET_MAX)


def field_scores(fl, fr, ndisp, field, vertical_range):
    """(S_L, S_R) [D,H,W] float32 where they are defined, zero elsewhere: offset_scores per offset the field holds,
    selected per entry."""
    H, W, _ = np.asarray(fl).shape
    F = clamped(field)
    gh, gw = F.shape
    assert 1 <= gh <= min(FIELD_MAX, H) and 1 <= gw <= min(FIELD_MAX, (W + 63) // 64)
    D = int(ndisp)
    per = {int(k): vo.offset_scores(fl, fr, D, int(k), vertical_range) for k in np.unique(F)}
    own = F[row_bands(H, gh)[:, None], column_bands(W, gw)[None, :]]              # F(h, w)
    sl, sr = np.zeros((D, H, W), np.float32), np.zeros((D, H, W), np.float32)
    for d in range(D):
        partner = own[:, np.minimum(np.arange(W) + d, W - 1)]                     # F(h, w + d)
        for k, (pl, pr) in per.items():
            sl[d][own == k] = pl[d][own == k]
            sr[d][partner == k] = pr[d][partner == k]
    return sl, sr


def compute_cost_volume_field(fl, fr, ndisp, field, vertical_range):
    """(lcv, rcv) [D,H,W] float32 of the definition."""
    return vr.fill_and_negate(*field_scores(fl, fr, ndisp, field, vertical_range))


def field_select(votes, H, row_step, max_offset, gh, gw):
    """(field int32 [gh, gw], totals uint64 [gh, gw, 2R + 1], offset, global totals uint64 [2R + 1])."""
    R, step, gh, gw = int(max_offset), int(row_step), int(gh), int(gw)
    votes = np.asarray(votes)
    n_rows, nb, nk = votes.shape
    rows = np.arange(step // 2, int(H), step)
    assert len(rows) == n_rows and nk == 2 * R + 1 and 1 <= gh <= min(FIELD_MAX, H) and 1 <= gw <= min(FIELD_MAX, nb)
    totals = np.zeros((gh, gw, nk), np.uint64)
    for i, h in enumerate(rows):
        for blk in range(nb):
            totals[h * gh // int(H), blk * gw // nb] += votes[i, blk].astype(np.uint64)
    offset, global_totals = vo.offset_select(votes, R)
    field = np.zeros((gh, gw), np.int32)
    for a in range(gh):
        for b in range(gw):
            field[a, b] = vo.offset_select(totals[a, b], R)[0] if totals[a, b].any() else offset
    return field, totals, offset, global_totals


def shear(image, ax, ay):
    """The image sheared by whole rows: pixel (h, x) shows row clip(h - dy(h, x), 0, H - 1), dy = rint(ax * (x - cx) / cx
    + ay * (h - cy) / cy) about the centre (cx, cy) = ((W - 1) / 2, (H - 1) / 2).  Returns (image, dy)."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    dy = np.rint(ax * (np.arange(W)[None, :] - cx) / cx + ay * (np.arange(H)[:, None] - cy) / cy).astype(np.int64)
    src = np.clip(np.arange(H)[:, None] - dy, 0, H - 1)
    return np.ascontiguousarray(image[src, np.arange(W)[None, :]]), dy
