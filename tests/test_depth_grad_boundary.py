"""CPU tests of the opt-in depth gradient's boundary (no GPU calls): the C entry point, its pybind and Python
surface exist and refuse bad input, and the scenes of the GPU parity tests (tests/depth_scenes.py) stay clear of
the blend's discrete rules, so those tests compare every element."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth_scenes as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization")
LIB = os.path.join(PKG, "libgs4d.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    return L


def test_header_declares_and_library_exports_backward_depth(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int gs4d_backward_depth\s*\(([^;]*)\);", text, flags=re.S)
    assert m, "gs4d.h does not declare gs4d_backward_depth"
    comment, params = m.group(1), m.group(2)
    # declared with its reference lines: the forward's depth accumulation and where the gradient is dropped
    assert "forward.cu" in comment and "__init__.py:100-101" in comment
    # gs4d_backward_ex's arguments plus dL_ddepth after dL_dpix
    ex = re.search(r"int gs4d_backward_ex\s*\(([^;]*)\);", text, flags=re.S).group(1)
    norm = lambda p: [re.sub(r"\s+", " ", a).strip() for a in p.split(",")]
    want = norm(ex)
    want.insert(want.index("const float *dL_dpix") + 1, "const float *dL_ddepth")
    assert norm(params) == want
    assert hasattr(lib, "gs4d_backward_depth")


def _args(P, R, dL_dpix, dL_ddepth):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [i(P), i(0), i(0), i(R), null, i(16), i(16), null, null, null, null, f(1.0), null, null, null, null, null,
            f(1.0), f(1.0), null, null, null, null, dL_dpix, dL_ddepth] + [null] * 9 + [null, null, i(0), null, i(0)]


def test_backward_depth_argument_errors_are_status_codes(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    for P, R in ((-1, 0), (4, -1)):
        assert lib.gs4d_backward_depth(*_args(P, R, some, some)) == 1
        assert b"backward" in lib.gs4d_last_error()
    # a missing gradient image is refused before any buffer is touched
    for pix, dep in ((some, null), (null, some)):
        assert lib.gs4d_backward_depth(*_args(4, 0, pix, dep)) == 1
        assert b"dL_ddepth" in lib.gs4d_last_error()
    # P == 0 is a no-op success, like gs4d_backward_ex
    assert lib.gs4d_backward_depth(*_args(0, 0, null, null)) == 0


def test_pybind_entry_exists_and_refuses_cpu_tensors():
    import diff_gaussian_rasterization as dgr
    assert hasattr(dgr._C, "rasterize_gaussians_backward_depth")
    e = torch.empty(0)
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        dgr._C.rasterize_gaussians_backward_depth(
            torch.ones(3), z, torch.zeros(4, dtype=torch.int32), e, z, torch.zeros(4, 4), 1.0, e, torch.eye(4),
            torch.eye(4), 0.5, 0.5, torch.zeros(3, 8, 8), torch.zeros(1, 8, 8), torch.zeros(4, 1, 3), 0,
            torch.zeros(3), torch.zeros(16, dtype=torch.uint8), 0, torch.zeros(16, dtype=torch.uint8),
            torch.zeros(16, dtype=torch.uint8), False)


def test_python_surface_is_opt_in():
    import inspect

    import diff_gaussian_rasterization as dgr
    from gs4d_train import config
    from gs4d_train.render import render
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    assert dgr.GaussianRasterizer(st).depth_grad is False
    assert dgr.GaussianRasterizer(st, depth_grad=True).depth_grad is True
    assert issubclass(dgr._RasterizeGaussiansDepth, torch.autograd.Function)
    assert inspect.signature(dgr.rasterize_gaussians).parameters["depth_grad"].default is False
    assert inspect.signature(render).parameters["depth_grad"].default is False
    assert config.optimization_params().lambda_depth == 0.0
    assert len(dgr.GaussianRasterizationSettings._fields) == 12  # the settings tuple does not change


@pytest.mark.parametrize("name", DS.NAMES)
def test_scene_preconditions(oracle, name):
    """No discrete rule bites on the parity scenes: no alpha above the 0.99 cap, none at the 1/255 threshold, no
    pixel near termination, the oracle's contributor counts, and not one near-threshold flag -- so the GPU tests
    exclude no element."""
    from gpu_helpers import o_bounds
    from oracle import parity as PAR
    sc = DS.scene(name)
    r = DS.reference(oracle, name)
    ref = r["ref"]
    assert ref["clamp099"] == 0 and ref["near_threshold"] == 0 and ref["min_T"] > 5e-3
    assert np.array_equal(ref["n_contrib"], r["export"]["n_contrib"])
    # the oracle's depth image is pinned by the restatement (the bar of tests/test_oracle.py)
    np.testing.assert_allclose(r["depth"], ref["depth"].detach().numpy(), atol=2e-5)
    g_c, _ = DS.upstream(name, "both")
    b = o_bounds(oracle, sc["s"], r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"],
                 use_sh=sc["use_sh"])
    assert int((np.asarray(b["gflag"]) != 0).sum()) == 0 and int((np.asarray(b["pflag"]) != 0).sum()) == 0
    lens = (r["export"]["ranges"][:, 1].astype(np.int64) - r["export"]["ranges"][:, 0]).reshape(-1)
    if name.startswith("dense"):
        assert lens.min() >= 65 and lens.max() > 128 and (lens % 2 == 1).any()  # several batches, odd lengths
    if name.startswith("hi"):
        assert (sc["s"]["opacities"] > 0.98).any() and sc["s"]["opacities"].max() < 0.99
    if name.startswith("rot"):
        v = sc["s"]["viewmatrix"].reshape(4, 4)
        assert np.abs(v[:3, 2] - np.array([0, 0, 1])).max() > 0.1  # the depth row is not the identity's
