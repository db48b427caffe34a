"""CPU: what the device-side ingest (csrc/ingest.hip) rests on, checked without a GPU - NumPy's summation order as the
kernel restates it, and the argument validation of the three entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ingest_helpers as ih

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mc-cnn-python_amd")


@pytest.mark.parametrize("shape", [s for s in ih.SHAPES if s != (2000, 3000)], ids=lambda s: "%dx%d" % s)
def test_stated_summation_order_is_numpys(shape):
    """The plain-Python statement of S (ingest_helpers.stated_sum: chunks of 8192, pairwise inside, left to right across)
    gives np.mean, np.std and the standardised image bit for bit.  If a NumPy changes its order or its buffer size this
    test says so before the GPU test does."""
    assert np.getbufsize() == ih.CHUNK
    for hist in ih.HISTOGRAMS:
        g8 = ih.image_u8(shape, hist, 1, seed=7)
        g = g8.astype(np.float32)
        mean, std, out = ih.stated_standardise(g8)
        with np.errstate(invalid="ignore", divide="ignore"):
            want_mean, want_std = np.mean(g, axis=(0, 1)), np.std(g, axis=(0, 1))
        assert want_mean.dtype == np.float32 and want_std.dtype == np.float32
        assert np.array_equal(ih.bits(mean), ih.bits(want_mean)), (shape, hist, mean, want_mean)
        assert np.array_equal(ih.bits(std), ih.bits(want_std)), (shape, hist, std, want_std)
        assert np.array_equal(ih.bits(out), ih.bits(ih.numpy_standardise(g8))), (shape, hist)


def test_stated_order_on_a_constant_image():
    g8 = np.full((40, 64), 77, np.uint8)
    _, _, out = ih.stated_standardise(g8)
    assert np.array_equal(ih.bits(out), ih.bits(ih.numpy_standardise(g8)))


@pytest.fixture(scope="module")
def lib():
    import _hipabi
    if not os.path.isfile(_hipabi.LIB_PATH):
        subprocess.check_call(["make", "-C", PKG, "-j4"])
    return _hipabi.load()


def test_ingest_argument_validation_without_gpu(lib):
    """The three entry points validate before they launch: codes and messages, no crash, no GPU needed."""
    import _hipabi as hip
    assert lib.mccnn_ingest_scratch_bytes(0, 10) == 0 and lib.mccnn_ingest_scratch_bytes(10, -1) == 0
    # two views x two sums x one float per chunk of 8192 pixels
    assert lib.mccnn_ingest_scratch_bytes(500, 750) >= 2 * 2 * 4 * ((500 * 750 + 8191) // 8192)
    assert lib.mccnn_ingest_scratch_bytes(1, 7) >= 16
    buf = ctypes.create_string_buffer(4096)          # host memory: never dereferenced, validation comes first
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.mccnn_ingest_scratch_bytes(40, 64)

    assert lib.mccnn_ingest_u8(None, 40, 64, 1, p, p, need, None) == hip.MCCNN_E_INVALID
    assert b"mccnn_ingest_u8: null pointer" in lib.mccnn_last_error_string()
    assert lib.mccnn_ingest_u8(p, 40, 64, 1, None, p, need, None) == hip.MCCNN_E_INVALID
    assert lib.mccnn_ingest_u8(p, 40, 64, 1, p, None, need, None) == hip.MCCNN_E_INVALID
    assert b"null pointer" in lib.mccnn_last_error_string()
    assert lib.mccnn_ingest_u8(p, 0, 64, 1, p, p, need, None) == hip.MCCNN_E_INVALID
    assert b"non-positive size" in lib.mccnn_last_error_string()
    for bad_c in (0, 2, 5, -3):
        assert lib.mccnn_ingest_u8(p, 40, 64, bad_c, p, p, need, None) == hip.MCCNN_E_INVALID
        assert b"expected 1 (grey), 3 (RGB) or 4 (RGBA)" in lib.mccnn_last_error_string()
    assert lib.mccnn_ingest_u8(p, 40, 64, 3, p, p, need - 1, None) == hip.MCCNN_E_SCRATCH
    assert b"mccnn_ingest_scratch_bytes(40, 64)" in lib.mccnn_last_error_string()

    assert lib.mccnn_ingest_u8_pair(p, None, 40, 64, 1, p, p, p, need, None) == hip.MCCNN_E_INVALID
    assert b"mccnn_ingest_u8_pair: null pointer" in lib.mccnn_last_error_string()
    assert lib.mccnn_ingest_u8_pair(p, p, 40, 64, 1, p, None, p, need, None) == hip.MCCNN_E_INVALID
    assert lib.mccnn_ingest_u8_pair(p, p, 40, -2, 1, p, p, p, need, None) == hip.MCCNN_E_INVALID
    assert b"non-positive size" in lib.mccnn_last_error_string()
    assert lib.mccnn_ingest_u8_pair(p, p, 40, 64, 2, p, p, p, need, None) == hip.MCCNN_E_INVALID
    assert lib.mccnn_ingest_u8_pair(p, p, 40, 64, 4, p, p, p, 0, None) == hip.MCCNN_E_SCRATCH
    assert b"scratch" in lib.mccnn_last_error_string()
    assert lib.mccnn_version() == 7                  # purely additive: the ABI version has not moved


def test_host_wrappers_refuse_what_is_not_a_byte_image():
    import torch
    import stereo_device as sd
    with pytest.raises(ValueError):
        sd._u8_image(torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(ValueError):
        sd._u8_image(torch.zeros((4,), dtype=torch.uint8))
    assert sd._u8_image(torch.zeros((4, 5), dtype=torch.uint8)) == (4, 5, 1)
    assert sd._u8_image(torch.zeros((4, 5, 3), dtype=torch.uint8)) == (4, 5, 3)
