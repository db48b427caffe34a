"""CPU: the envelope of full-resolution pairs (2 <= D <= 1024, D <= W - 2, volumes past 4 GiB) as the host states it -
StereoMatcher's workspace footprint - and the refusals outside it, which return before anything is launched."""
import ctypes

import pytest


def test_workspace_bytes_states_the_allocations():
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W, D = 1988, 2880, 800
    n = sd.workspace_bytes(H, W, D)
    vols = 4 * H * W * 800 * 4
    assert 73e9 < vols < 74e9
    extra = (5 * lib.mccnn_sgm_scratch_bytes(H, W, D) + 2 * lib.mccnn_support_bytes(H, W) + 7 * H * W * 4
             + 2 * lib.mccnn_cbca_prog_bytes(D, H, W))
    assert n == vols + extra
    assert lib.mccnn_cbca_prog_bytes(D, H, W) == 0          # 2880 columns: cbca_hwd_kernel, no program buffers
    assert sd.workspace_bytes(H, W, D, pairs_in_flight=3) == 3 * n
    # a padded pitch (Dp = 4 * ceil(D / 4)) and the program buffers where the assembly aggregation runs
    h, w, d = 12, 1100, 1022
    progs = lib.mccnn_cbca_prog_bytes(d, h, w)
    assert progs > 0
    got = sd.workspace_bytes(h, w, d)
    assert got == 4 * h * w * 1024 * 4 + (5 * lib.mccnn_sgm_scratch_bytes(h, w, d) + 2 * lib.mccnn_support_bytes(h, w)
                                          + 7 * h * w * 4 + 2 * progs)
    assert sd.workspace_bytes(h, w, d, cbca_kernel="hwd") == got - 2 * progs
    assert sd.workspace_bytes(h, w, d, pixel_major=False) == got - 2 * progs
    # the largest supported shape: 3072 x 2048 x 1024, four volumes of 25.8 GB
    assert 103e9 < sd.workspace_bytes(2048, 3072, 1024) < 104e9


@pytest.mark.parametrize("H,W,D,what", [(10, 2000, 1025, "1024"), (10, 2000, 1, "2, 1024"), (10, 600, 599, "W=600"),
                                        (0, 600, 64, "empty")])
def test_workspace_bytes_refuses_outside_the_envelope(H, W, D, what):
    import stereo_device as sd
    with pytest.raises(ValueError, match=what):
        sd.workspace_bytes(H, W, D)


def test_abi_refuses_outside_the_envelope_before_launching():
    """D > 1024 for SGM and the pixel-major cost volume, D > W - 2 for the cost volume: MCCNN_E_UNSUPPORTED from the
    argument checks (the pointers are never dereferenced: nothing reaches a device)."""
    import _hipabi as hip
    lib = hip.load()
    fake = ctypes.c_void_p(4096)
    vols = (ctypes.c_void_p * 2)(4096, None)
    sides = (ctypes.c_int * 2)(hip.MCCNN_SIDE_LEFT, 0)
    for D in (1025, 2048):
        rc = lib.mccnn_sgm_pass_flagged(vols, sides, 1, D, 4, 3000, 1, 0, 1.0, 2.0, 4.0, 8.0, fake, 1 << 30, None)
        assert rc == hip.MCCNN_E_UNSUPPORTED
        assert b"1024" in lib.mccnn_last_error_string()
        rc = lib.mccnn_sgm_flags(fake, fake, D, 4, 3000, 1, 0, 0.08, fake, 1 << 30, None)
        assert rc == hip.MCCNN_E_UNSUPPORTED
        rc = lib.mccnn_cost_volume_hwd(fake, fake, 4, 3000, 64, D, fake, fake, hip.MCCNN_CV_EXACT, None)
        assert rc == hip.MCCNN_E_UNSUPPORTED
    rc = lib.mccnn_cost_volume_hwd(fake, fake, 4, 1025, 64, 1024, fake, fake, hip.MCCNN_CV_EXACT, None)
    assert rc == hip.MCCNN_E_UNSUPPORTED
