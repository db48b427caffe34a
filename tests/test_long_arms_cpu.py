"""No GPU: the route decision for cbca_distance 15 to 32 (stereo_device.aggregation_route - the one function
StereoMatcher, workspace_bytes' callers and process_functional read), the footprint it states, and the C ABI's new
entry points in the header and the ctypes table."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def sd():
    import stereo_device
    return stereo_device


def test_route_function(sd):
    import _hipabi as hip
    ref, sep = hip.MCCNN_CBCA_REFERENCE_ORDER, hip.MCCNN_CBCA_SEPARABLE
    W, D = 750, 256
    for dist in range(15, 33):
        assert sd.aggregation_route(dist, W, D, ref, None, "auto") == "hwd_long"
        assert sd.aggregation_route(dist, 3000, 1024, ref, {"both_view_support": False}, "auto") == "hwd_long"
        assert sd.aggregation_route(dist, W, D, ref, None, "plane_major") == "plane_major"
        assert sd.aggregation_route(dist, W, D, ref, {"both_view_support": True}, "auto") == "plane_major"
        assert sd.aggregation_route(dist, W, D, sep, None, "auto") == "plane_major"
    for dist in range(1, 15):
        # exactly as before: the aggregation programs where they encode the shape, cbca_hwd_kernel otherwise
        assert sd.aggregation_route(dist, W, D, ref, None, "auto") == "prog"
        assert sd.aggregation_route(dist, 2880, 64, ref, None, "auto") == "hwd"          # wider than a program op encodes
        assert sd.aggregation_route(dist, W, D, ref, None, "auto", cbca_kernel="hwd") == "hwd"
        assert sd.aggregation_route(dist, W, D, ref, None, "plane_major") == "plane_major"
        assert sd.aggregation_route(dist, W, D, ref, {"both_view_support": True}, "auto") == "plane_major"
    for dist in (0, 33, 40):
        with pytest.raises(ValueError):
            sd.aggregation_route(dist, W, D, ref, None, "auto")
    with pytest.raises(ValueError):
        sd.aggregation_route(28, W, D, ref, None, "hwd")


def test_route_states_the_workspace_without_program_buffers(sd):
    import _hipabi as hip
    H, W, D = 500, 750, 256
    route = sd.aggregation_route(28, W, D, hip.MCCNN_CBCA_REFERENCE_ORDER, None, "auto", H=H)
    assert sd.route_cbca_kernel(route) == "hwd"
    assert sd.route_cbca_kernel(sd.aggregation_route(14, W, D, hip.MCCNN_CBCA_REFERENCE_ORDER, None, "auto", H=H)) == "auto"
    progs = 2 * int(hip.load().mccnn_cbca_prog_bytes(D, H, W))
    assert progs > 0
    assert sd.workspace_bytes(H, W, D, True, "auto") - sd.workspace_bytes(H, W, D, True, "hwd") == progs


def test_header_declares_and_binding_binds_the_long_arm_entry_points():
    import _hipabi as hip
    header = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    lib = hip.load()
    for name, nargs in (("mccnn_cbca_iter_hwd_long", 8), ("mccnn_cbca_iter_hwd_long_pair", 11)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header)
        assert m, "%s is not declared in include/mccnn.h" % name
        assert len(m.group(1).split(",")) == nargs
        assert len(hip.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    assert hip.MCCNN_ABI_VERSION == 7 and lib.mccnn_version() == 7
