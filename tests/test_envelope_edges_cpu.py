"""CPU: the grid of shapes at the edges of check_envelope (envelope_grid.py) - what it holds, that the oracle's whole
chain is defined on every one of them, how many of its expected maps can tell a wrong kernel from a right one, and
that check_envelope refuses the neighbours just outside."""
import numpy as np
import pytest

import envelope_grid as grid


def test_grid_lies_inside_the_envelope_and_holds_the_named_edges():
    import stereo_device as sd
    assert len(grid.FULL) == 138 and len(set(grid.FULL)) == 138
    assert len(grid.REDUCED) == 19 and len(set(grid.REDUCED)) == 19
    assert set(grid.REDUCED) <= set(grid.FULL)
    for H in grid.HEIGHTS:
        assert len(grid.shapes_of_height(H)) == len(grid.WIDTH_DISPARITIES), H
    for H, W, D in grid.FULL:
        sd.check_envelope(H, W, D)
        assert H >= 1 and 2 <= D <= 1024 and D <= W - 2, grid.name((H, W, D))
    for which in (grid.FULL, grid.REDUCED):
        assert any(H == 1 for H, W, D in which)
        assert any(D == W - 2 for H, W, D in which)
        assert any(D == 2 for H, W, D in which)
        assert any(sd.hwd_pitch(D) != D for H, W, D in which)
        assert any(D > 256 for H, W, D in which)
    assert any(D == 1024 for H, W, D in grid.FULL)
    assert any(H < 5 and W < 5 for H, W, D in grid.FULL)          # narrower and lower than the 5x5 windows
    assert {13, 14, 15, 28, 29, 30} <= {H for H, W, D in grid.FULL}


def test_oracle_chain_is_finite_on_every_shape():
    """Seeded random unit features through the oracle's whole chain: every stage of every shape is finite (a NaN target
    would hide a difference: the comparison canonicalises NaN payloads)."""
    import oracle
    for shape in grid.FULL:
        H, W, D = shape
        L, R = grid.make_pair(shape)
        assert np.isfinite(L).all() and np.isfinite(R).all(), grid.name(shape)
        fl, fr = grid.unit_features(shape)
        final, st = oracle.match_from_features(L, R, fl, fr, D, return_all=True)
        assert final.shape == (H, W) and final.dtype == np.float32, grid.name(shape)
        for stage, res in st.items():
            for a in (res if isinstance(res, tuple) else (res,)):
                assert np.isfinite(a).all(), "%s: %s is not finite" % (grid.name(shape), stage)


def test_most_expected_maps_are_not_constant(net_layers):
    """A constant expected map says little about the kernel that wrote it (the images at most 7 wide give one: 53 of the
    138 final maps, 51 of the WTA maps, with the checkpoint's features and these seeds).  The floor: at least 80 of the
    138 expected final maps vary (85 measured).  Should a change of `synthetic` move the count, the seeds change, not
    the floor.  The GPU tests compare the volumes, which are never constant, for every shape."""
    import oracle
    varying, constant = 0, []
    for shape in grid.FULL:
        L, R = grid.make_pair(shape)
        final = oracle.match_pair(L, R, shape[2], net_layers)
        assert np.isfinite(final).all(), grid.name(shape)
        if np.unique(final).size > 1:
            varying += 1
        else:
            constant.append(grid.name(shape))
    assert varying >= 80, "%d of %d expected final maps vary; constant: %s" % (varying, len(grid.FULL), constant)


@pytest.mark.parametrize("H,W,D,what", [(5, 20, 1, r"outside \[2, 1024\]"), (5, 20, 19, "at least ndisp \\+ 2 = 21"),
                                        (5, 2000, 1025, r"outside \[2, 1024\]"), (0, 20, 2, "empty image"),
                                        (1, 3, 2, "at least ndisp \\+ 2 = 4")])
def test_check_envelope_refuses_the_neighbours_outside(H, W, D, what):
    import stereo_device as sd
    with pytest.raises(ValueError, match=what):
        sd.check_envelope(H, W, D)
