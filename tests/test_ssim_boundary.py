"""CPU tests of the SSIM / D-SSIM boundary (no GPU calls): include/gs4d_train.h declares the entry points, the
built library exports them, argument errors come back as status 1 before any HIP call, and gs4d_train.kernels
lists the Python names."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs4d_train.h")
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
NAMES = ("gs4d_ssim_scratch_bytes", "gs4d_ssim_forward", "gs4d_ssim_backward", "gs4d_l1_dssim_loss_grad")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    return ctypes.CDLL(LIB)


def test_header_declares_the_ssim_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs4d_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared, sorted(set(NAMES) - declared)
    assert "utils/loss_utils.py:36-66" in open(HEADER).read()


def test_library_exports_the_ssim_entry_points(lib):
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing


def test_ssim_argument_errors_are_status_codes(lib):
    null = ctypes.c_void_p(0)
    i = ctypes.c_int
    one = (ctypes.c_float * 4)()  # host memory: never touched, an argument error returns before any HIP call
    for dims in ((-1, 3, 8, 8), (1, -3, 8, 8), (1, 3, -8, 8), (1, 3, 8, -8), (-1, -3, 8, 8)):
        d = [i(v) for v in dims]
        assert lib.gs4d_ssim_forward(*d, one, one, null, one, one, one, null) == 1, dims
        assert lib.gs4d_ssim_backward(*d, one, one, one, one, i(0), one, null) == 1, dims
        assert lib.gs4d_l1_dssim_loss_grad(*d, one, one, ctypes.c_float(0.2), ctypes.c_float(1.0), one, one, one, one,
                                           one, null) == 1, dims
    d = [i(1), i(3), i(8), i(8)]
    assert lib.gs4d_ssim_forward(*d, null, one, null, one, one, one, null) == 1      # x
    assert lib.gs4d_ssim_forward(*d, one, one, null, null, one, one, null) == 1      # mean
    assert lib.gs4d_ssim_forward(*d, one, one, null, one, one, null, null) == 1      # scratch
    assert lib.gs4d_ssim_backward(*d, one, one, null, one, i(0), one, null) == 1     # maps
    assert lib.gs4d_l1_dssim_loss_grad(*d, one, one, ctypes.c_float(0.2), ctypes.c_float(1.0), null, one, one, one, one,
                                       null) == 1                                    # the maps workspace
    lib.gs4d_ssim_scratch_bytes.restype = ctypes.c_size_t
    assert lib.gs4d_ssim_scratch_bytes(i(-1), i(3), i(8), i(8)) == 0
    assert lib.gs4d_ssim_scratch_bytes(i(2), i(3), i(70), i(101)) >= 2 * 2 * 8 * 3 * 3 * 4


def test_kernels_module_lists_the_ssim_names():
    src = open(os.path.join(ROOT, "4dgaussians-fast-train_amd", "gs4d_train", "kernels.py")).read()
    all_list = re.search(r"__all__\s*=\s*\[(.*?)\]", src, flags=re.S).group(1)
    names = re.findall(r'"([A-Za-z0-9_]+)"', all_list)
    assert "ssim" in names and "l1_dssim_loss_and_grad" in names
    from gs4d_train import kernels
    assert "ssim" in kernels.__all__ and "l1_dssim_loss_and_grad" in kernels.__all__
    assert callable(kernels.ssim) and callable(kernels.l1_dssim_loss_and_grad)
