"""CPU tests of the HyperNeRF / DyCheck shape (F, W) = (48, 128) at the library's boundary (no GPU call): the C entry
points accept it and still refuse their neighbours, include/gs4d_train.h lists it with the reference's lines, the
presets hold arguments/hypernerf/default.py's and arguments/dycheck/default.py's values, a model built from them has
the 48-wide field and the (128, 48) first layer, and on CPU tensors the inference path stays the torch formulation."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs4d_train.h")
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")

POS, SCALES, ROT, OPACITY, SHS = range(5)
ROLE_N = {POS: 3, SCALES: 3, ROT: 4, OPACITY: 1, SHS: 48}


class Args(ctypes.Structure):
    """gs4d_deform_infer_args"""
    _fields_ = ([(n, ctypes.c_int) for n in ("P", "F", "W", "K", "k", "activate")] +
                [(n, ctypes.c_void_p) for n in ("feat", "wf", "bf", "w1", "b1")] +
                [("role", ctypes.c_int * 5), ("n", ctypes.c_int * 5), ("w2", ctypes.c_void_p * 5),
                 ("b2", ctypes.c_void_p * 5)] +
                [(n, ctypes.c_void_p) for n in ("xyz", "s", "r", "o", "f_dc", "f_rest", "means", "scales", "rot", "opac",
                                                "shs")])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    L.gs4d_deform_infer.argtypes = [ctypes.POINTER(Args), ctypes.c_void_p]
    L.gs4d_deform_infer.restype = ctypes.c_int
    L.gs4d_feature_relu_forward.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    L.gs4d_feature_relu_forward.restype = ctypes.c_int
    return L


_HOST = (ctypes.c_char * 64)()  # host memory, never touched: these calls return before any HIP call
_PTR = (ctypes.addressof(_HOST) + 15) & ~15


def _args(P=0, F=48, W=128, K=16, roles=(POS, SCALES, ROT, OPACITY, SHS)):
    a = Args()
    a.P, a.F, a.W, a.K, a.k, a.activate = P, F, W, K, len(roles), 1
    for name in ("feat", "wf", "bf", "w1", "b1", "xyz", "s", "r", "o", "f_dc", "f_rest", "means", "scales", "rot", "opac",
                 "shs"):
        setattr(a, name, _PTR)
    for i, r in enumerate(roles):
        a.role[i], a.n[i], a.w2[i], a.b2[i] = r, ROLE_N[r], _PTR, _PTR
    return a


@pytest.mark.parametrize("roles", [(POS, SCALES, ROT, OPACITY, SHS), (POS, SCALES, ROT), (ROT,)])
def test_deform_infer_accepts_48_128_with_no_points(lib, roles):
    assert lib.gs4d_deform_infer(ctypes.byref(_args(roles=roles)), None) == 0


def test_feature_relu_forward_accepts_48_128_with_no_points(lib):
    assert lib.gs4d_feature_relu_forward(0, 48, 128, None, _PTR, _PTR, None, None) == 0
    assert lib.gs4d_feature_relu_forward(0, 48, 128, None, None, _PTR, None, None) == 1  # w = NULL
    for Fin, Fout in ((48, 64), (64, 128), (16, 128), (48, 256), (0, 0)):
        assert lib.gs4d_feature_relu_forward(0, Fin, Fout, None, _PTR, _PTR, None, None) == 1, (Fin, Fout)


def test_neighbouring_shapes_stay_refused_with_a_text(lib):
    for F, W in ((32, 256), (16, 128), (64, 128), (48, 64), (0, 0)):
        assert lib.gs4d_deform_infer(ctypes.byref(_args(P=8, F=F, W=W)), None) == 1, (F, W)
        msg = lib.gs4d_last_error()
        assert msg.startswith(b"deform_infer:") and b"(F, W)" in msg, (F, W, msg)
        for shape in (b"(32, 128)", b"(48, 128)", b"(64, 64)", b"(32, 64)"):  # the four it is built for
            assert shape in msg, (shape, msg)


def test_header_lists_the_shape_and_cites_the_reference():
    raw = open(HEADER).read()
    feature = raw[raw.index("The deformation field's first layer, backward"):raw.index("int gs4d_feature_relu_forward(")]
    infer = raw[raw.index("The deformation network at inference"):raw.index("typedef struct gs4d_deform_infer_args")]
    for block in (feature, infer):
        assert "(48, 128)" in block
        assert "arguments/hypernerf/default.py:5-10" in block and "arguments/dycheck/default.py:5-10" in block


HIDDEN = dict(kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 16,
                              "resolution": [64, 64, 64, 150]},
              multires=[1, 2, 4], defor_depth=1, net_width=128, plane_tv_weight=0.0002, time_smoothness_weight=0.001,
              l1_time_planes=0.0001)
OPT = dict(batch_size=2, coarse_iterations=3000, densify_until_iter=10_000, opacity_reset_interval=300000)


@pytest.mark.parametrize("name,iterations", [("hypernerf", 14_000), ("dycheck", 60_000)])
def test_presets_hold_the_reference_values(name, iterations):
    from gs4d_train import config
    hidden, opt = getattr(config, name.upper() + "_HIDDEN"), getattr(config, name.upper() + "_OPT")
    assert hidden == HIDDEN and "render_process" not in hidden
    assert opt == {**OPT, "iterations": iterations}
    hyper, o = getattr(config, name)()
    assert vars(hyper) == vars(config.model_hidden_params(**HIDDEN))
    assert vars(o) == vars(config.optimization_params(**OPT, iterations=iterations))
    assert hyper.no_do is True and hyper.no_dshs is True and not (hyper.no_dx or hyper.no_ds or hyper.no_dr)


def _cpu_model(name, P=40, seed=0):
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    hyper, _ = getattr(config, name)()
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=False)
    rnd = lambda *s: torch.nn.Parameter(torch.randn(*s))
    g._xyz, g._scaling, g._rotation, g._opacity = rnd(P, 3), rnd(P, 3), rnd(P, 4), rnd(P, 1)
    g._features_dc, g._features_rest = rnd(P, 1, 3), rnd(P, 15, 3)
    g.active_sh_degree = 3
    with torch.no_grad():
        for level in g._deformation.deformation_net.grid.grids:
            for p in level:  # the time planes start at exactly 1: move every plane off its initial value
                p.copy_(torch.rand_like(p) * 0.9 + 0.1)
    return g


@pytest.mark.parametrize("name", ["hypernerf", "dycheck"])
def test_preset_model_has_the_48_wide_field_and_stays_unfused_on_the_cpu(name):
    from gs4d_train import infer
    from gs4d_train.deformation import _FeatureReLU
    g = _cpu_model(name)
    net = g._deformation.deformation_net
    assert net.grid.feat_dim == 48 and len(net.grid.grids) == 3
    assert tuple(net.state_dict()["feature_out.0.weight"].shape) == (128, 48) and len(net.feature_out) == 1
    assert (net.grid.feat_dim, net.W) in _FeatureReLU.shapes and (48, 128) in infer._SHAPES
    assert [n for n, _ in infer._active(net.args)] == ["pos_deform", "scales_deform", "rotations_deform"]
    # CPU tensors: the served shape must not put the model on the HIP path
    state = infer.prepare(g)
    assert state.fused is False
    P = g._xyz.shape[0]
    with torch.no_grad():
        time = torch.full((P, 1), float(np.float32(0.37)))
        want = g._deformation(g._xyz, g._scaling, g._rotation, g._opacity, g.get_features, time)
    got = infer.state_at_time(state, 0.37, activate=False)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], g._xyz.detach())  # the field does deform
    assert torch.equal(got[3], g._opacity.detach()) and torch.equal(got[4], g.get_features.detach())  # no head
