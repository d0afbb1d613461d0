"""CPU tests of the inference path's boundary (no GPU calls): include/gs4d_train.h declares gs4d_deform_infer with
its reference lines, the built library exports it, argument errors come back as status 1 with a gs4d_last_error
text before any HIP call, gs4d_train.infer exposes its six names, _C.deform_infer refuses CPU tensors, and
ply.save_frame writes a per-frame 3DGS file that reads back (fallback formulation on the CPU, bitwise the torch
module's values, the reference's undeformed-opacity quirk included)."""
import ctypes
import os
import re

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
    return L


_HOST = (ctypes.c_char * 64)()  # host memory, never touched: an argument error returns before any HIP call
_PTR = (ctypes.addressof(_HOST) + 15) & ~15  # 16-byte aligned, as the ABI asks of feat, the weights, rot and shs


def _args(P=8, F=32, W=128, K=16, roles=(POS, SCALES, ROT, OPACITY, SHS), ns=None, **over):
    a = Args()
    a.P, a.F, a.W, a.K, a.k, a.activate = P, F, W, K, len(roles), 1
    for name in ("feat", "wf", "bf", "w1", "b1", "xyz", "s", "r", "o", "f_dc", "f_rest", "means", "scales", "rot", "opac",
                 "shs"):
        setattr(a, name, _PTR)
    for i, r in enumerate(roles[:5]):
        a.role[i] = r
        a.n[i] = ROLE_N.get(r, 3) if ns is None else ns[i]
        a.w2[i] = _PTR
        a.b2[i] = _PTR
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_header_declares_deform_infer_and_cites_the_reference():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert "gs4d_deform_infer" in set(re.findall(r"\b(gs4d_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"typedef struct gs4d_deform_infer_args\s*\{", text)
    assert "scene/deformation.py:51-55,73-78,97-146" in raw
    assert "gaussian_renderer/__init__.py:94-99" in raw


def test_library_exports_deform_infer(lib):
    assert hasattr(lib, "gs4d_deform_infer")


def _refused(lib, a, what):
    st = lib.gs4d_deform_infer(ctypes.byref(a), None)
    assert st == 1, (what, st)
    msg = lib.gs4d_last_error()
    assert msg.startswith(b"deform_infer:") and len(msg) > len(b"deform_infer: "), (what, msg)
    return msg


def test_argument_errors_are_status_1_with_a_text(lib):
    assert b"P" in _refused(lib, _args(P=-1), "P < 0")
    for F, W in ((32, 256), (16, 128), (64, 128), (48, 64), (0, 0)):
        assert b"(F, W)" in _refused(lib, _args(F=F, W=W), f"(F, W) = ({F}, {W})")
    assert b"heads" in _refused(lib, _args(roles=()), "k = 0")
    assert b"heads" in _refused(lib, _args(k=6), "k = 6")
    assert b"twice" in _refused(lib, _args(roles=(POS, ROT, POS)), "a repeated role")
    _refused(lib, _args(roles=(POS, 7)), "a role that does not exist")
    assert b"n =" in _refused(lib, _args(roles=(POS, ROT), ns=(3, 3)), "rot with n = 3")
    assert b"n =" in _refused(lib, _args(roles=(SHS,), ns=(45,)), "shs with n = 45")
    assert b"K = 16" in _refused(lib, _args(K=4), "an shs head with K = 4")
    for name in ("feat", "wf", "bf", "w1", "b1", "xyz", "s", "r", "o", "f_dc", "f_rest", "means", "scales", "rot", "opac",
                 "shs"):
        _refused(lib, _args(**{name: None}), f"null {name}")
    for arr in ("w2", "b2"):
        a = _args()
        getattr(a, arr)[2] = None
        _refused(lib, a, f"null {arr}[2]")
    assert lib.gs4d_deform_infer(None, None) == 1


def test_supported_arguments_with_no_points_are_a_no_op(lib):
    for F, W in ((32, 128), (64, 64), (32, 64)):
        assert lib.gs4d_deform_infer(ctypes.byref(_args(P=0, F=F, W=W)), None) == 0
    # the D-NeRF default's heads (no shs head: any K), one head only
    assert lib.gs4d_deform_infer(ctypes.byref(_args(P=0, F=64, W=64, K=4, roles=(POS, SCALES, ROT))), None) == 0
    assert lib.gs4d_deform_infer(ctypes.byref(_args(P=0, roles=(ROT,))), None) == 0


def test_infer_module_exposes_its_six_names():
    from gs4d_train import infer
    names = ("prepare", "state_at_time", "get_state_at_time", "render_view", "render_set", "evaluate")
    assert tuple(infer.__all__) == names
    assert all(callable(getattr(infer, n)) for n in names)


def test_bindings_refuse_cpu_tensors():
    from gs4d_train import _C
    W, F, P = 64, 32, 4
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="GPU"):
        _C.deform_infer(z(P, F), z(W, F), z(W), z(W, W), z(W), [z(4, W)], [z(4)], [ROT], z(P, 3), z(P, 3), z(P, 4),
                        z(P, 1), z(P, 1, 3), z(P, 15, 3), True)
    with pytest.raises(RuntimeError, match="GPU"):
        _C.hexplane_forward_packed(z(P, 4), z(6 * 4 * 4 * 4), 4, [4] * 6, [4] * 6, torch.zeros(P, dtype=torch.int32))


def _cpu_model(P=50, seed=0, **over):
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    hyper = config.model_hidden_params(**{**config.DNERF_HIDDEN, "no_do": False, "no_dshs": False, **over})
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


def test_save_frame_round_trip_on_the_cpu(tmp_path):
    from gs4d_train import infer, ply
    from gs4d_train.gaussians import GaussianModel
    g = _cpu_model()
    P = g.get_xyz.shape[0]
    state = infer.prepare(g)
    assert state.fused is False  # CPU tensors: the torch formulation
    cam = type("Cam", (), {"time": 0.37})()
    path = str(tmp_path / "gaussian_pertimestamp" / "time_00000.ply")
    ply.save_frame(path, state, cam)
    with torch.no_grad():
        time = torch.full((P, 1), float(np.float32(0.37)))
        want = g._deformation(g._xyz, g._scaling, g._rotation, g._opacity, g.get_features, time)
    m3, sc, rot, op, sh = want
    assert not torch.equal(op, g._opacity)  # the opacity head is on: the quirk below is visible
    el = ply.read_ply(path)
    assert list(el) == ply.attribute_names(3, 45)
    col = lambda names: torch.tensor(np.stack([el[k] for k in names], 1))
    assert torch.equal(col(["x", "y", "z"]), m3)
    assert not np.any(col(["nx", "ny", "nz"]).numpy())
    assert torch.equal(col([f"scale_{i}" for i in range(3)]), sc)
    assert torch.equal(col([f"rot_{i}" for i in range(4)]), rot)
    assert torch.equal(col(["opacity"]), g._opacity.detach())  # utils/render_utils.py:18: the UNDEFORMED opacity
    assert torch.equal(col([f"f_dc_{i}" for i in range(3)]), sh[:, :1].transpose(1, 2).flatten(1))
    assert torch.equal(col([f"f_rest_{i}" for i in range(45)]), sh[:, 1:].transpose(1, 2).flatten(1))
    g2 = GaussianModel(3, g._deformation.deformation_net.args, fused=False)
    ply.load_gaussians(path, g2, device="cpu")
    for got, exp in ((g2._xyz, m3), (g2._scaling, sc), (g2._rotation, rot), (g2._opacity, g._opacity),
                     (g2.get_features, sh)):
        assert torch.equal(got.detach(), exp.detach())
    # a time instead of a camera; get_state_at_time is what the file holds
    ply.save_frame(str(tmp_path / "t.ply"), state, 0.37)
    assert open(path, "rb").read() == open(str(tmp_path / "t.ply"), "rb").read()
    got = infer.get_state_at_time(state, cam)
    for a, b in zip(got, (m3, sc, rot, g._opacity.detach(), sh)):
        assert torch.equal(a, b)


def test_state_is_a_capture_on_the_cpu():
    from gs4d_train import infer
    g = _cpu_model(P=20, seed=1)
    state = infer.prepare(g)
    before = infer.state_at_time(state, 0.5)
    with torch.no_grad():
        g._deformation.deformation_net.grid.grids[0][2].mul_(1.5)
        g._deformation.deformation_net.pos_deform[3].weight.add_(0.25)
    after = infer.state_at_time(state, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    fresh = infer.state_at_time(infer.prepare(g), 0.5)
    assert not torch.equal(fresh[0], before[0])
    coarse = infer.state_at_time(infer.prepare(g, "coarse"), 0.5)
    assert torch.equal(coarse[0], g._xyz.detach()) and torch.equal(coarse[1], torch.exp(g._scaling.detach()))
