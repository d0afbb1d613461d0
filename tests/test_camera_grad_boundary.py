"""CPU tests of the opt-in camera gradient's boundary (no GPU calls): the C entry exists and reports argument errors as
status codes, the Python surface defaults to off, the fp64 reference (tests/camera_grad_refs.py) is the tested
restatement with camera leaves and obeys the two rigid-motion identities, the parity bar of
tests/test_camera_grad_gpu.py bites, PoseRefiner's contract, and the scenes' margins.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import camera_grad_refs as CR
import torch_restatement as TR
from gpu_helpers import o_bounds
from test_rule_branches_boundary import CLAMP_MARGIN, TERM_MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    return L


def _decl(text, name):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\s*\(([^;]*)\);", text, flags=re.S)
    assert m, f"{name} is not declared (with its comment)"
    return m.group(1), [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]


def test_header_declares_and_library_and_binding_export_the_entry(lib):
    import diff_gaussian_rasterization as dgr
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    _, aa = _decl(text, "gs4d_backward_aa")
    comment, params = _decl(text, "gs4d_backward_camera")
    assert params == aa + ["float *dL_dcamera"]
    for word in ("35", "dL/dviewmatrix", "dL/dprojmatrix", "dL/dcampos", "atomics", "P == 0", "NULL"):
        assert word in comment, word
    assert hasattr(lib, "gs4d_backward_camera")
    assert hasattr(dgr._C, "rasterize_gaussians_backward_camera")


def _args(P, R, dL_dpix, opacities, aa, cam):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [i(P), i(0), i(0), i(R), null, i(16), i(16), null, null, null, null, f(1.0), null, null, null, null, null,
            f(1.0), f(1.0), null, null, null, null, dL_dpix, null, null] + [null] * 9 + [null] + \
        [null, null, i(0), null, i(0), opacities, i(aa), cam]


def test_argument_errors_are_status_codes(lib):
    """each of these returns before any HIP call, so the test needs no GPU"""
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gs4d_backward_camera(*_args(4, 0, some, some, 0, null)) == 1       # no output for the gradient
    assert lib.gs4d_last_error().startswith(b"backward_camera")
    assert lib.gs4d_backward_camera(*_args(0, 0, null, null, 0, null)) == 1       # ... for P == 0 as well
    assert lib.gs4d_backward_camera(*_args(4, 0, some, null, 1, some)) == 1       # antialiasing needs the opacities
    assert lib.gs4d_last_error().startswith(b"backward_camera")
    assert lib.gs4d_backward_camera(*_args(4, 0, some, null, 0, some)) == 1       # ... without it, the buffers
    assert lib.gs4d_last_error().startswith(b"backward:")
    for P, R in ((-1, 0), (4, -1)):
        assert lib.gs4d_backward_camera(*_args(P, R, some, some, 1, some)) == 1
        assert lib.gs4d_last_error().startswith(b"backward:")


def test_python_surface_is_opt_in():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import config, infer
    from gs4d_train.camera import Camera
    from gs4d_train.render import render
    from gs4d_train.train import train_step
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    assert len(dgr.GaussianRasterizationSettings._fields) == 12
    assert dgr.GaussianRasterizer(st).camera_grad is False
    assert dgr.GaussianRasterizer(st, camera_grad=True).camera_grad is True
    for fn in (dgr.rasterize_gaussians, render):
        assert inspect.signature(fn).parameters["camera_grad"].default is False, fn
    for fn in (render, infer.render_view):
        assert inspect.signature(fn).parameters["camera_tensors"].default is None, fn
    assert inspect.signature(train_step).parameters["pose"].default is None
    assert config.optimization_params().pose_lr == 0.0
    assert len(dgr._FUNCTIONS) == 8 and len(dgr.__all__) == 11
    assert inspect.signature(Camera.__init__).parameters["uid"].default is None


def test_camera_tensors_travel_as_inputs_only_when_on(monkeypatch):
    """off: the Function gets today's nine (or ten) arguments; on: the switch and the settings' three camera tensors
    follow them"""
    import diff_gaussian_rasterization as dgr
    seen = []
    for fn in set(dgr._FUNCTIONS.values()):
        monkeypatch.setattr(fn, "apply", staticmethod(lambda *a, _n=fn.__name__: seen.append((_n, a[9:]))))
    V, Pm, c = torch.eye(4), torch.ones(4, 4), torch.zeros(3)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, V, Pm, 0, c, False, False)
    for key, fn in dgr._FUNCTIONS.items():
        for aa in (False, True):
            seen.clear()
            dgr.rasterize_gaussians(*range(8), st, depth_grad=key[0], alpha=key[1], absgrad=key[2], antialiasing=aa)
            assert seen == [(fn.__name__, (True,) if aa else ())]
            seen.clear()
            dgr.rasterize_gaussians(*range(8), st, depth_grad=key[0], alpha=key[1], absgrad=key[2], antialiasing=aa,
                                    camera_grad=True)
            assert len(seen) == 1 and seen[0][0] == fn.__name__ and seen[0][1][0] is aa
            assert seen[0][1][1] is V and seen[0][1][2] is Pm and seen[0][1][3] is c and len(seen[0][1]) == 4


def test_train_step_refuses_data_parallel_with_a_refiner():
    from gs4d_train import config
    from gs4d_train.pose import PoseRefiner
    from gs4d_train.train import train_step
    opt = config.optimization_params(pose_lr=1e-3)
    with pytest.raises(ValueError, match="not reduced across ranks"):
        train_step(None, [], opt, None, 1, None, data_parallel=True, pose=PoseRefiner(1, "cpu"))


# ---- the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.NAMES)
def test_detached_camera_leaves_give_the_tested_restatement_bitwise(oracle, name):
    sc, r = CR.scene(name), CR.reference(oracle, name)
    s, ex = sc["s"], r["export"]
    kw = dict(use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"])
    mine = CR.forward_autograd(s, ex["point_list"], ex["ranges"], s["sh_degree"], camera_leaves=False, **kw)
    plain = TR.forward_autograd(s, ex["point_list"], ex["ranges"], s["sh_degree"], **kw)
    for k in ("color", "depth", "Tfinal"):
        assert torch.equal(mine[k], plain[k]), k
        assert torch.equal(r["ref"][k], plain[k]), k            # and leaves do not change the values
    g_c, g_d, g_a = CR.upstream(oracle, name, "all")
    leaves = ["ndc_off", "rgb", "opac", "means", "cov3", "scales", "rots"] + (["shs"] if sc["use_sh"] else [])
    for ref in (mine, r["ref"]):
        a = torch.autograd.grad(CR.loss_of(ref, g_c, g_d, g_a), [ref[k] for k in leaves], retain_graph=True)
        b = torch.autograd.grad(CR.loss_of(plain, g_c, g_d, g_a), [plain[k] for k in leaves], retain_graph=True)
        for k, x, y in zip(leaves, a, b):
            assert torch.equal(x, y), k


@pytest.mark.parametrize("name,aa", [(n, False) for n in CR.NAMES] + [("cam_sh", True), ("cam_colors", True)])
def test_translation_identity(oracle, name, aa):
    """moving the camera rigidly is moving every mean the other way:
    sum_j dL/dV[3, j] V[a, j] + sum_j dL/dPm[3, j] Pm[a, j] - dL/dc[a] = sum_i dL/dmeans3D_i[a]"""
    ref = CR.reference(oracle, name, aa)["ref"]
    cr = CR.camera_ref(oracle, name, "all", aa)
    lhs, rhs = CR.translation_residual(ref["V"].detach().numpy(), ref["Pm"].detach().numpy(), cr["dV"], cr["dPm"],
                                       cr["dc"], cr["dmeans"])
    assert np.abs(rhs).max() > 1.0
    np.testing.assert_allclose(lhs, rhs, rtol=0, atol=1e-10 * np.abs(rhs).max())


def _cross_matrix(g):
    """G (3, 3) -> the vector of its antisymmetric part's generator: sum over the rotation generators' action"""
    return np.array([g[1, 2] - g[2, 1], g[2, 0] - g[0, 2], g[0, 1] - g[1, 0]])


@pytest.mark.parametrize("name", CR.COLOR_NAMES)
def test_rotation_identity(oracle, name):
    """rotating the camera about the world origin is rotating the scene the other way.  With row vectors p_h V, a
    world rotation m -> m R, Sigma -> R^T Sigma R equals V -> R V (rows 0..2), Pm -> R Pm; for R = exp(eps K) the
    two first-order changes of the loss, sum_ab K[a][b] G[a][b], have the same antisymmetric part of
        G = dL/dV[:3] V[:3]^T + dL/dPm[:3] Pm[:3]^T     and     G = sum_i m_i^T dL/dm_i + 2 Sigma_i dL/dSigma_i
    (colors_precomp: no view direction, so the camera centre does not enter)."""
    ref = CR.reference(oracle, name)["ref"]
    cr = CR.camera_ref(oracle, name, "all")
    V, Pm = ref["V"].detach().numpy(), ref["Pm"].detach().numpy()
    cam_side = cr["dV"][:3, :] @ V[:3, :].T + cr["dPm"][:3, :] @ Pm[:3, :].T
    m = ref["means"].detach().numpy()
    Sig = ref["cov3"].detach().numpy()
    dS = 0.5 * (cr["dcov"] + cr["dcov"].transpose(0, 2, 1))
    scene_side = np.einsum("pa,pb->ab", m, cr["dmeans"]) + 2.0 * np.einsum("pac,pcb->ab", Sig, dS)
    a, b = _cross_matrix(cam_side), _cross_matrix(scene_side)
    assert np.abs(b).max() > 1.0
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-9 * np.abs(b).max())


def test_the_parity_bar_bites(oracle):
    """on at least one scene every family of terms has an element whose sum is >= 10 bars of that element: a
    backward that drops a family cannot pass the parity test"""
    best = {f: 0.0 for f in CR.FAMILIES}
    for name in CR.NAMES:
        cr = CR.camera_ref(oracle, name, "color")
        bar = CR.bar(cr["A"])
        ratios = {f: float((np.abs(v) / bar).max()) for f, v in cr["families"].items()}
        print(f"[camera-bites] {name}: max |family sum| / bar " + " ".join(f"{f}={v:.1f}" for f, v in ratios.items()),
              flush=True)
        if all(v >= 10.0 for v in ratios.values()):
            best = ratios
    assert all(v >= 10.0 for v in best.values()), best
    # and the W-term, which the reference never forms, is not a small correction of the t-term
    cr = CR.camera_ref(oracle, "cam_colors", "color")
    assert np.abs(cr["families"]["W"]).max() > 0.1 * np.abs(cr["families"]["t"]).max()


# ---- PoseRefiner -----------------------------------------------------------------------------------------------
def _camera():
    return CR.scene("cam_sh")["s"]["camera"]


def test_pose_refiner_at_zero_returns_the_camera_bitwise():
    from gs4d_train.pose import PoseRefiner
    cam = _camera()
    V, Pm, c = PoseRefiner(1, "cpu").tensors(cam)
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    assert torch.equal(bits(V), bits(cam.world_view_transform))
    assert torch.equal(bits(Pm), bits(cam.full_proj_transform))
    assert torch.equal(bits(c), bits(cam.camera_center))
    assert V.requires_grad and Pm.requires_grad and c.requires_grad
    cam.uid = 2
    try:
        r = PoseRefiner(3, "cpu")
        with torch.no_grad():
            r.trans[1] = 1.0                        # another camera's row
        assert torch.equal(bits(r.tensors(cam)[0]), bits(cam.world_view_transform))
        with pytest.raises(ValueError):
            PoseRefiner(2, "cpu").tensors(cam)
    finally:
        cam.uid = None
    with pytest.raises(ValueError):
        PoseRefiner(2, "cpu").tensors(cam)         # no uid, several rows


def test_pose_refiner_is_the_camera_frame_perturbation():
    """p_view' = R(omega) p_view + tau, Pm' = V' projection, and c' is the point V' sends to the origin (fp64)"""
    from gs4d_train.pose import PoseRefiner
    cam = _camera()
    r = PoseRefiner(1, "cpu", dtype=torch.float64)
    omega = np.array([0.3, -0.2, 0.5])
    tau = np.array([0.1, 0.2, -0.3])
    with torch.no_grad():
        r.rot[0] = torch.tensor(omega)
        r.trans[0] = torch.tensor(tau)
    V, Pm, c = (t.detach().numpy() for t in r.tensors(cam))
    V0 = cam.world_view_transform.double().numpy()
    th = np.linalg.norm(omega)
    K = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    p = np.array([[0.4, 1.0, 2.0, 1.0], [-1.0, 0.3, 5.0, 1.0]])
    np.testing.assert_allclose((p @ V)[:, :3], (p @ V0)[:, :3] @ R.T + tau, atol=1e-12)
    np.testing.assert_allclose(V[:, 3], [0, 0, 0, 1], atol=0)
    # the camera's own Pm and c are float32 roundings of V0 projection and of the centre: 1e-6 covers them
    np.testing.assert_allclose(Pm, V @ cam.projection_matrix.double().numpy(), atol=1e-6)
    np.testing.assert_allclose((np.append(c, 1.0) @ V)[:3], 0, atol=1e-6)


def test_pose_refiner_jacobian_at_zero_is_finite_and_matches_central_differences():
    from gs4d_train.pose import PoseRefiner
    cam = _camera()
    r = PoseRefiner(1, "cpu", dtype=torch.float64)

    def f(x):
        r.rot, r.trans = x[:3].reshape(1, 3), x[3:].reshape(1, 3)
        return torch.cat([t.reshape(-1) for t in r.tensors(cam)])
    x0 = torch.zeros(6, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(f, x0)
    assert J.shape == (35, 6) and torch.isfinite(J).all() and J.abs().max() > 0.5
    h = 1e-6
    eye = torch.eye(6, dtype=torch.float64)
    with torch.no_grad():
        Jn = torch.stack([(f(x0 + h * eye[i]) - f(x0 - h * eye[i])) / (2 * h) for i in range(6)], 1)
    assert (J - Jn).abs().max() < 1e-8
    # across the series / closed-form switch the rotation is continuous to rounding
    from gs4d_train.pose import rotation_minus_identity
    d = torch.tensor([0.06, -0.05, 0.062], dtype=torch.float64)
    d = d / d.norm()
    below, above = rotation_minus_identity(d * 0.0999999), rotation_minus_identity(d * 0.1000001)
    assert (below - above).abs().max() < 1e-6 and (below - above).abs().max() > 0


# ---- the scenes ------------------------------------------------------------------------------------------------
def preconditions(O, sc, r, g_c):
    """the conditions under which every element can be compared with fp64 (also used to look for seeds)"""
    ref, ex, s = r["ref"], r["export"], sc["s"]
    b = o_bounds(O, s, r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    assert int((np.asarray(b["gflag"]) != 0).sum()) == 0 and int((np.asarray(b["pflag"]) != 0).sum()) == 0
    assert ref["near_threshold"] == 0
    assert np.array_equal(ref["n_contrib"], ex["n_contrib"])
    assert ref["clamp_margin"] >= CLAMP_MARGIN, ref["clamp_margin"]
    assert not ref["nonpd"][r["radii"] > 0].any() and ref["n_power_rejected"] == 0
    assert ref["clamp099"] == 0 and ref["n_terminated"] == 0 and ref["term_margin"] >= TERM_MARGIN


@pytest.mark.parametrize("name", CR.NAMES)
def test_scene_preconditions(oracle, name):
    sc, r = CR.scene(name), CR.reference(oracle, name)
    s, ref = sc["s"], r["ref"]
    P = s["means3D"].shape[0]
    assert P <= 300 and s["W"] <= 70 and s["H"] <= 45
    preconditions(oracle, sc, r, CR.upstream(oracle, name, "color")[0])
    vis = r["radii"] > 0
    rotated = np.abs(s["viewmatrix"].reshape(4, 4)[:3, :3] - np.eye(3)).max() > 0.1
    if name == "cam_sh":
        assert sc["use_sh"] and s["sh_degree"] == 3 and rotated and ref["n_clamped"] == 0 and vis.sum() >= 50
    if name == "cam_colors":
        assert not sc["use_sh"] and rotated
    if name in ("cam_clamp", "cam_colors"):
        fx, fy = s["W"] / (2 * s["tanfovx"]), s["H"] / (2 * s["tanfovy"])
        assert abs(fx - fy) > 5 and rotated
        assert int((ref["clamped"] & vis).sum()) >= 15, int((ref["clamped"] & vis).sum())
    if name == "cam_dense":
        lens = r["export"]["ranges"][:, 1].astype(np.int64) - r["export"]["ranges"][:, 0]
        assert P == 300 and lens.sum() >= 1000 and vis.sum() >= 250      # about 16 waves of records
    if name == "cam_behind":
        t = (np.c_[s["means3D"].astype(np.float64), np.ones(P)] @ s["viewmatrix"].astype(np.float64).reshape(4, 4))
        behind = t[:, 2] <= 0.2
        assert np.array_equal(np.nonzero(behind)[0], np.arange(0, P, 3)) and not vis[behind].any()
        assert vis.sum() >= 30 and rotated


@pytest.mark.parametrize("mode", ["colors", "sh"])
@pytest.mark.parametrize("P", CR.EDGE_P)
def test_edge_scene_preconditions(oracle, P, mode):
    sc = CR.edge_scene(P, mode)
    r = CR.make_reference(oracle, sc)
    assert sc["s"]["W"] == 32 and sc["s"]["H"] == 32 and sc["s"]["means3D"].shape[0] == P
    preconditions(oracle, sc, r, np.ones((3, 32, 32), np.float32))
    assert r["ref"]["n_clamped"] == 0
    if P > 1:
        assert (r["radii"] > 0).sum() >= P - 8
