"""CPU tests of the opt-in alpha image's boundary (no GPU calls): the three C entry points, their pybind and
Python surface exist, default to off and refuse bad input; the scenes of tests/alpha_scenes.py have the properties
the GPU tests (tests/test_alpha_gpu.py) rely on; and train_step's mask plumbing, with a torch stand-in renderer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import alpha_scenes as AS

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


def _decl(text, name):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:size_t \w+\s*\([^;]*\);\s*)?int " + name + r"\s*\(([^;]*)\);", text,
                  flags=re.S)
    assert m, f"{name} is not declared (with its comment)"
    return m.group(1), [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]


def test_headers_declare_and_library_exports_the_entry_points(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    comment, params = _decl(text, "gs4d_alpha_image")
    # declared with its reference lines: where the forward stores final_T, and that no such image is returned
    assert "forward.cu:373" in comment and "__init__.py:98" in comment
    assert params == ["int width", "int height", "const char *image_buffer", "float *out_alpha", "void *stream"]
    # gs4d_backward_depth's arguments plus dL_dalpha after dL_ddepth
    _, want = _decl(text, "gs4d_backward_depth")
    want.insert(want.index("const float *dL_ddepth") + 1, "const float *dL_dalpha")
    comment, params = _decl(text, "gs4d_backward_aux")
    assert params == want and "backward.cu" in comment
    train = open(os.path.join(ROOT, "include", "gs4d_train.h")).read()
    _, params = _decl(train, "gs4d_aux_loss_grad")
    assert params == ["int64_t n", "const float *depth", "const float *alpha", "const float *gt_depth",
                      "const float *gt_mask", "float w_depth", "float w_mask", "float *loss", "float *dL_ddepth",
                      "float *dL_dalpha", "void *scratch", "void *stream"]
    for name in ("gs4d_alpha_image", "gs4d_backward_aux", "gs4d_aux_loss_grad", "gs4d_aux_loss_scratch_bytes"):
        assert hasattr(lib, name), name
    # the existing entries keep their signatures (tests/test_depth_grad_boundary.py pins gs4d_backward_depth's)
    assert hasattr(lib, "gs4d_backward_depth") and hasattr(lib, "gs4d_backward_ex")


def _aux_args(P, R, dL_dpix, dL_ddepth, dL_dalpha):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [i(P), i(0), i(0), i(R), null, i(16), i(16), null, null, null, null, f(1.0), null, null, null, null, null,
            f(1.0), f(1.0), null, null, null, null, dL_dpix, dL_ddepth, dL_dalpha] + [null] * 9 + \
        [null, null, i(0), null, i(0)]


def test_argument_errors_are_status_codes(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    i = ctypes.c_int
    # gs4d_alpha_image: an empty image or a NULL pointer
    for w, h, img, out in ((0, 4, some, some), (4, 0, some, some), (-1, 4, some, some), (4, 4, null, some),
                           (4, 4, some, null)):
        assert lib.gs4d_alpha_image(i(w), i(h), img, out, null) == 1
        assert lib.gs4d_last_error().startswith(b"alpha_image")
    # gs4d_backward_aux: bad sizes and a missing dL_dpix, with either, both or no auxiliary gradient
    for P, R in ((-1, 0), (4, -1)):
        assert lib.gs4d_backward_aux(*_aux_args(P, R, some, some, some)) == 1
        assert lib.gs4d_last_error().startswith(b"backward")
    for dep, alp in ((some, some), (some, null), (null, some), (null, null)):
        assert lib.gs4d_backward_aux(*_aux_args(4, 0, null, dep, alp)) == 1
        assert lib.gs4d_last_error().startswith(b"backward")
    # P == 0 succeeds at once
    assert lib.gs4d_backward_aux(*_aux_args(0, 0, null, null, null)) == 0
    # gs4d_aux_loss_grad: n < 1, a NULL loss / scratch, a NULL image of a term that is present
    lib.gs4d_aux_loss_scratch_bytes.restype = ctypes.c_size_t
    assert lib.gs4d_aux_loss_scratch_bytes(ctypes.c_int64(3150)) >= 24 * 2
    f, n = ctypes.c_float, ctypes.c_int64
    call = lambda n_, d, a, gd, gm, loss, dd, da, scr: lib.gs4d_aux_loss_grad(n(n_), d, a, gd, gm, f(1.0), f(1.0),
                                                                              loss, dd, da, scr, null)
    assert call(0, some, some, some, some, some, some, some, some) == 1
    assert call(4, some, some, some, some, null, some, some, some) == 1
    assert call(4, some, some, some, some, some, some, some, null) == 1
    assert call(4, null, some, some, some, some, some, some, some) == 1
    assert call(4, some, some, some, some, some, null, some, some) == 1
    assert call(4, some, null, some, some, some, some, some, some) == 1
    assert call(4, some, some, some, some, some, some, null, some) == 1


def test_pybind_entries_exist_and_refuse_cpu_tensors():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import _C as TC
    from gs4d_train import kernels
    assert hasattr(dgr._C, "alpha_image") and hasattr(dgr._C, "rasterize_gaussians_backward_aux")
    assert hasattr(TC, "aux_loss_grad") and "aux_loss_and_grad" in kernels.__all__
    with pytest.raises(RuntimeError):
        dgr._C.alpha_image(torch.zeros(8 * 8 * 8 + 1024, dtype=torch.uint8), 8, 8)
    e = torch.empty(0)
    z = torch.zeros(4, 3)
    for g_d, g_a in ((torch.zeros(1, 8, 8), torch.zeros(1, 8, 8)), (e, torch.zeros(1, 8, 8)), (e, e)):
        with pytest.raises(RuntimeError):
            dgr._C.rasterize_gaussians_backward_aux(
                torch.ones(3), z, torch.zeros(4, dtype=torch.int32), e, z, torch.zeros(4, 4), 1.0, e, torch.eye(4),
                torch.eye(4), 0.5, 0.5, torch.zeros(3, 8, 8), g_d, g_a, torch.zeros(4, 1, 3), 0, torch.zeros(3),
                torch.zeros(16, dtype=torch.uint8), 0, torch.zeros(16, dtype=torch.uint8),
                torch.zeros(16, dtype=torch.uint8), False)
    with pytest.raises(RuntimeError):
        kernels.aux_loss_and_grad(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.ones(1, 4, 4),
                                  torch.ones(1, 4, 4), 1.0, 1.0)


def test_python_surface_is_opt_in():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import config
    from gs4d_train.render import render
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    assert dgr.GaussianRasterizer(st).alpha is False and dgr.GaussianRasterizer(st).depth_grad is False
    r = dgr.GaussianRasterizer(st, depth_grad=True, alpha=True)
    assert r.alpha is True and r.depth_grad is True
    assert issubclass(dgr._RasterizeGaussiansAux, torch.autograd.Function)
    assert inspect.signature(dgr.rasterize_gaussians).parameters["alpha"].default is False
    assert inspect.signature(dgr.rasterize_gaussians).parameters["depth_grad"].default is False
    assert inspect.signature(render).parameters["alpha"].default is False
    assert inspect.signature(render).parameters["depth_grad"].default is False
    assert config.optimization_params().lambda_mask == 0.0 and config.optimization_params().lambda_depth == 0.0
    assert len(dgr.GaussianRasterizationSettings._fields) == 12  # the settings tuple does not change


def test_scene_preconditions(oracle):
    """opaque has terminated walks next to mostly empty pixels; sparse has empty tiles next to covered pixels;
    behind has Gaussians and not one instance"""
    o = AS.reference(oracle, "opaque")
    assert o["nr"] > 0
    assert int((o["final_T"] < 2e-4).sum()) >= 100 and int((o["final_T"] > 0.5).sum()) >= 50
    s = AS.scene("sparse")["s"]
    r = AS.reference(oracle, "sparse")
    empty = AS.tile_is_empty(r, s["H"], s["W"])
    lens = r["ranges"][:, 1].astype(np.int64) - r["ranges"][:, 0]
    assert int((lens == 0).sum()) >= 8 and empty.any()
    assert int((r["n_contrib"] > 0).sum()) >= 1
    assert np.all(r["final_T"][r["n_contrib"] == 0] == 1.0)
    b = AS.reference(oracle, "behind")
    assert AS.scene("behind")["s"]["means3D"].shape[0] > 0 and b["nr"] == 0 and np.all(b["final_T"] == 1.0)


# ---- train_step's mask plumbing, on the CPU with a torch stand-in renderer (the style of test_train_dp_gloo.py) ----
H = W = 6


def _model(P=120, seed=0):
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    hyper, opt = config.dnerf()
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=False)
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    g._xyz = torch.nn.Parameter(f32(rng.normal(size=(P, 3))))
    g._features_dc = torch.nn.Parameter(f32(rng.normal(size=(P, 1, 3))))
    g._features_rest = torch.nn.Parameter(f32(rng.normal(size=(P, 15, 3))))
    g._scaling = torch.nn.Parameter(f32(rng.normal(-3, 0.5, size=(P, 3))))
    g._rotation = torch.nn.Parameter(f32(rng.normal(size=(P, 4))))
    g._opacity = torch.nn.Parameter(f32(rng.normal(size=(P, 1))))
    g.max_radii2D = torch.zeros(P)
    g._deformation_table = torch.ones(P, dtype=torch.bool)
    g.spatial_lr_scale = 1.0
    g.training_setup(opt)
    return g, hyper, opt


def _views(n):
    from types import SimpleNamespace
    gen = torch.Generator().manual_seed(7)
    out = []
    for i in range(n):
        cam = SimpleNamespace(A=torch.randn(3, 2, generator=gen) + 2.0, time=i / n)
        out.append((cam, torch.rand(3, H, W, generator=gen), torch.rand(1, H, W, generator=gen)))
    return out  # (camera, gt, mask)


class _Renderer:
    """render()'s dict from a small differentiable splatter; records the keyword arguments of every call and takes
    alpha / depth_grad like render() -- and no other keyword"""

    def __init__(self):
        self.calls = []

    def __call__(self, cam, pc, debug, bg, stage="coarse", **kw):
        assert set(kw) <= {"alpha", "depth_grad"}
        self.calls.append((cam, dict(kw)))
        xyz = pc.get_xyz
        ss = torch.zeros_like(xyz, requires_grad=True) + 0
        ss.retain_grad()
        m2 = xyz @ cam.A + ss[:, :2]
        s = pc.get_scaling.max(dim=1).values * 20
        col = pc.get_features[:, 0, :] * 0.28 + 0.5
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32),
                                indexing="ij")
        pix = torch.stack([xx.reshape(-1), yy.reshape(-1)], 1)
        wgt = pc.get_opacity[:, 0][:, None] * torch.exp(-((pix[None] - m2[:, None]) ** 2).sum(-1)
                                                        / (2 * s[:, None] ** 2 + 1))
        tot = wgt.sum(0)
        img = (wgt[:, :, None] * col[:, None, :]).sum(0) / (1 + tot[:, None])
        radii = torch.ceil(3 * s).to(torch.int32)
        out = {"render": img.t().reshape(3, H, W), "viewspace_points": ss, "visibility_filter": radii > 0,
               "radii": radii, "depth": torch.zeros(1, H, W)}
        if kw.get("alpha"):
            out["alpha"] = (tot / (1 + tot)).reshape(1, H, W)
        return out


def _step(views, lambda_mask, lambda_depth=0.0):
    from gs4d_train.train import train_step
    g, hyper, opt = _model()
    opt.lambda_mask, opt.lambda_depth = lambda_mask, lambda_depth
    r = _Renderer()
    loss = train_step(g, views, opt, hyper, 1, torch.ones(3), stage="coarse", fused_loss=False, render_fn=r)
    params = {k: getattr(g, k).detach().clone() for k in ("_xyz", "_features_dc", "_features_rest", "_scaling",
                                                          "_rotation", "_opacity")}
    return loss, params, r


def test_train_step_mask_plumbing():
    trip = _views(2)
    pairs = [(c, gt) for c, gt, _ in trip]
    # view 0 carries a mask (with no depth), view 1 is a pair; view 1's mask is (H, W)
    views = [(trip[0][0], trip[0][1], None, trip[0][2]), pairs[1]]
    lam = 0.7
    l_mask, p_mask, r = _step(views, lam)
    l_pair, p_pair, r0 = _step(pairs, lam)
    assert [kw for _, kw in r.calls] == [{"alpha": True}, {}]      # alpha=True only where a mask is used
    assert [kw for _, kw in r0.calls] == [{}, {}]
    g, _, _ = _model()
    alpha = _Renderer()(trip[0][0], g, False, None, alpha=True)["alpha"].detach()
    term = lam * (alpha - trip[0][2]).abs().mean() / 2              # share / len(mine) = 1 / 2 views
    assert float(term) > 1e-3
    assert abs(float(l_mask) - float(l_pair + term)) <= 1e-6 * abs(float(l_mask))
    assert not torch.equal(p_mask["_xyz"], p_pair["_xyz"])          # the term reached the parameters
    # an (H, W) mask is accepted, and a depth in slot 2 is used only under lambda_depth
    both = [(trip[0][0], trip[0][1], torch.rand(1, H, W) + 0.5, trip[0][2][0]), pairs[1]]
    l_hw, _, r1 = _step(both, lam)
    assert float(l_hw) == float(l_mask) and [kw for _, kw in r1.calls] == [{"alpha": True}, {}]
    _, _, r2 = _step(both, lam, lambda_depth=0.5)
    assert [kw for _, kw in r2.calls] == [{"depth_grad": True, "alpha": True}, {}]
    # lambda_mask = 0 with 4-tuple views: the pair-view step bit for bit, and render_fn sees no new keyword
    quads = [(c, gt, None, m) for c, gt, m in trip]
    l0, p0, r3 = _step(quads, 0.0)
    lp, pp, _ = _step(pairs, 0.0)
    assert [kw for _, kw in r3.calls] == [{}, {}]
    assert torch.equal(l0, lp)
    for k in pp:
        assert torch.equal(p0[k], pp[k]), k
