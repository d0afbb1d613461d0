"""CPU tests of the opt-in absolute screen-space gradient's boundary (no GPU calls): the C entry point, its pybind and
Python surface exist and default to off, a missing output is a status code, the fp64 reference of the GPU tests
(tests/absgrad_refs.py) agrees with the existing restatement, and train_step's densify_absgrad plumbing, with a
torch stand-in renderer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

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


def test_header_declares_and_library_exports_the_entry_point(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    # gs4d_backward_aux's arguments plus abs_dmean2D after the last gradient output
    _, want = _decl(text, "gs4d_backward_aux")
    want.insert(want.index("float *dL_drot") + 1, "float *abs_dmean2D")
    comment, params = _decl(text, "gs4d_backward_absgrad")
    assert params == want
    # the formula's source lines, and the record layout: float 9 is W3, floats 10 and 11 the absolute sums, full
    assert "backward.cu:541-546" in comment and "float 9" in comment and "floats 10 and 11" in comment
    assert "full" in comment
    assert hasattr(lib, "gs4d_backward_absgrad")
    for name in ("gs4d_backward_ex", "gs4d_backward_depth", "gs4d_backward_aux"):
        assert hasattr(lib, name), name


def _args(P, R, dL_dpix, abs_out):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [i(P), i(0), i(0), i(R), null, i(16), i(16), null, null, null, null, f(1.0), null, null, null, null, null,
            f(1.0), f(1.0), null, null, null, null, dL_dpix, null, null] + [null] * 9 + [abs_out] + \
        [null, null, i(0), null, i(0)]


def test_argument_errors_are_status_codes(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    # a NULL abs_dmean2D is an error whatever P is; bad sizes and a missing dL_dpix as in gs4d_backward_aux
    for P in (0, 4):
        assert lib.gs4d_backward_absgrad(*_args(P, 0, some, null)) == 1
        assert lib.gs4d_last_error().startswith(b"backward_absgrad")
    for P, R in ((-1, 0), (4, -1)):
        assert lib.gs4d_backward_absgrad(*_args(P, R, some, some)) == 1
    assert lib.gs4d_backward_absgrad(*_args(4, 0, null, some)) == 1
    assert lib.gs4d_last_error().startswith(b"backward")
    assert lib.gs4d_backward_absgrad(*_args(0, 0, null, some)) == 0  # P == 0 succeeds at once


def test_pybind_entry_exists_and_refuses_cpu_tensors():
    import diff_gaussian_rasterization as dgr
    assert hasattr(dgr._C, "rasterize_gaussians_backward_absgrad")
    e = torch.empty(0)
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        dgr._C.rasterize_gaussians_backward_absgrad(
            torch.ones(3), z, torch.zeros(4, dtype=torch.int32), e, z, torch.zeros(4, 4), 1.0, e, torch.eye(4),
            torch.eye(4), 0.5, 0.5, torch.zeros(3, 8, 8), e, e, torch.zeros(4, 1, 3), 0, torch.zeros(3),
            torch.zeros(16, dtype=torch.uint8), 0, torch.zeros(16, dtype=torch.uint8),
            torch.zeros(16, dtype=torch.uint8), False)


def test_python_surface_is_opt_in():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import config
    from gs4d_train.render import render
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    assert inspect.signature(dgr.GaussianRasterizer.__init__).parameters["absgrad"].default is False
    assert dgr.GaussianRasterizer(st).absgrad is False
    r = dgr.GaussianRasterizer(st, depth_grad=True, alpha=True, absgrad=True)
    assert r.absgrad is True and r.alpha is True and r.depth_grad is True
    assert inspect.signature(dgr.rasterize_gaussians).parameters["absgrad"].default is False
    assert inspect.signature(render).parameters["absgrad"].default is False
    assert config.optimization_params().densify_absgrad is False
    for fn in (dgr._RasterizeGaussiansAbs, dgr._RasterizeGaussiansAbsDepth, dgr._RasterizeGaussiansAuxAbs,
               dgr._RasterizeGaussiansAuxDepthAbs):
        assert issubclass(fn, torch.autograd.Function)
    assert len(dgr.GaussianRasterizationSettings._fields) == 12  # the settings tuple does not change


def test_flags_select_one_of_eight_distinct_functions(monkeypatch):
    """rasterize_gaussians hands its nine arguments to the Function of its (depth_grad, alpha, absgrad) triple; no
    Function runs here (every .apply is a recorder)"""
    import diff_gaussian_rasterization as dgr
    table = {(False, False, False): "_RasterizeGaussians",
             (True, False, False): "_RasterizeGaussiansDepth",
             (False, True, False): "_RasterizeGaussiansAux",
             (True, True, False): "_RasterizeGaussiansAuxDepth",
             (False, False, True): "_RasterizeGaussiansAbs",
             (True, False, True): "_RasterizeGaussiansAbsDepth",
             (False, True, True): "_RasterizeGaussiansAuxAbs",
             (True, True, True): "_RasterizeGaussiansAuxDepthAbs"}
    classes = [getattr(dgr, n) for n in table.values()]
    assert len(set(classes)) == 8
    for c in classes:
        assert issubclass(c, torch.autograd.Function)
    assert len(dgr.__all__) == 11 and set(table.values()) < set(dgr.__all__)
    for n in dgr.__all__:
        assert getattr(dgr, n) is not None, n
    calls = []
    for n, c in zip(table.values(), classes):
        monkeypatch.setattr(c, "apply", staticmethod(lambda *a, n=n: calls.append((n, a)) or n))
    args = tuple(object() for _ in range(9))
    for (depth_grad, alpha, absgrad), want in table.items():
        assert dgr.rasterize_gaussians(*args, depth_grad=depth_grad, alpha=alpha, absgrad=absgrad) == want
        assert calls[-1][0] == want and all(x is y for x, y in zip(calls[-1][1], args)) and len(calls[-1][1]) == 9
    assert dgr.rasterize_gaussians(*args) == "_RasterizeGaussians"  # every flag defaults to off
    assert len(calls) == 9
    # the module passes its three flags on
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    z = torch.zeros(4, 3)
    for triple, want in table.items():
        r = dgr.GaussianRasterizer(st, depth_grad=triple[0], alpha=triple[1], absgrad=triple[2])
        assert r(means3D=z, means2D=z, opacities=z[:, :1], shs=z, scales=z, rotations=z) == want


def test_reference_signed_sum_is_the_restatements_gradient(oracle):
    """the per-(pixel, slot) leaf's gradient, scatter-added with its sign, is the existing restatement's ndc_off
    gradient to 1e-12 (asserted inside the helper); its absolute scatter-sum dominates it and is not the same"""
    import absgrad_refs as AR
    import depth_scenes as DS
    name = "small0"
    g_c, g_d = DS.upstream(name, "both")
    want = DS.autograd_grads(oracle, name, g_c, g_d)[0]
    absg, signed = AR.absgrad_reference(AR.scene_forward(oracle, name), g_c, g_d, signed_want=want)
    assert absg.shape == want.shape == (60, 2) and np.abs(want).max() > 0
    assert np.all(np.abs(signed) <= absg * (1 + 1e-12))
    assert np.any(absg > 2 * np.abs(signed))
    radii = DS.reference(oracle, name)["radii"]
    assert not np.any(absg[radii == 0])


# ---- train_step's plumbing, on the CPU with a torch stand-in renderer (the style of test_alpha_boundary.py) ----
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
    return [(SimpleNamespace(A=torch.randn(3, 2, generator=gen) + 2.0, time=i / n), torch.rand(3, H, W, generator=gen))
            for i in range(n)]


class _Renderer:
    """render()'s dict from a small differentiable splatter; with absgrad=True a hook leaves a recognisable
    .absgrad on viewspace_points when its gradient arrives (2 |grad| + 1), unless `forget` is set"""

    def __init__(self, forget=False):
        self.calls, self.forget, self.abs = [], forget, []

    def __call__(self, cam, pc, debug, bg, stage="coarse", **kw):
        assert set(kw) <= {"absgrad"}
        self.calls.append(dict(kw))
        xyz = pc.get_xyz
        ss = torch.zeros_like(xyz, requires_grad=True)
        m2 = xyz @ cam.A + ss[:, :2]
        s = pc.get_scaling.max(dim=1).values * 20
        col = pc.get_features[:, 0, :] * 0.28 + 0.5
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32),
                                indexing="ij")
        pix = torch.stack([xx.reshape(-1), yy.reshape(-1)], 1)
        wgt = pc.get_opacity[:, 0][:, None] * torch.exp(-((pix[None] - m2[:, None]) ** 2).sum(-1)
                                                        / (2 * s[:, None] ** 2 + 1))
        img = (wgt[:, :, None] * col[:, None, :]).sum(0) / (1 + wgt.sum(0)[:, None])
        radii = torch.ceil(3 * s).to(torch.int32)
        radii[::5] = 0
        if kw.get("absgrad") and not self.forget:
            def hook(g, ss=ss):
                ss.absgrad = 2 * g.abs() + 1
                self.abs.append(ss.absgrad)
            ss.register_hook(hook)
        return {"render": img.t().reshape(3, H, W), "viewspace_points": ss, "visibility_filter": radii > 0,
                "radii": radii, "depth": torch.zeros(1, H, W)}


def _step(views, r, **over):
    from gs4d_train.train import train_step
    g, hyper, opt = _model()
    for k, v in over.items():
        setattr(opt, k, v)
    loss = train_step(g, views, opt, hyper, 1, torch.ones(3), stage="coarse", fused_loss=False, render_fn=r)
    params = {k: getattr(g, k).detach().clone() for k in ("_xyz", "_features_dc", "_features_rest", "_scaling",
                                                          "_rotation", "_opacity")}
    return loss, params, g


def test_train_step_densify_absgrad_plumbing():
    views = _views(2)
    r_on, r_off, r_none = _Renderer(), _Renderer(), _Renderer()
    l_on, p_on, g_on = _step(views, r_on, densify_absgrad=True)
    l_off, p_off, g_off = _step(views, r_off, densify_absgrad=False)
    l_none, p_none, g_none = _step(views, r_none)
    # every view is rendered with absgrad=True under the flag, and render_fn sees no new keyword without it
    assert r_on.calls == [{"absgrad": True}] * 2 and r_off.calls == [{}] * 2 and r_none.calls == [{}] * 2
    # the statistics took the views' summed .absgrad in place of the summed .grad
    assert len(r_on.abs) == 2
    total = r_on.abs[0] + r_on.abs[1]
    vis = torch.ones(total.shape[0], dtype=torch.bool)  # the stand-in's radii: positive scales, every 5th set to 0
    vis[::5] = False
    want = torch.where(vis[:, None], torch.norm(total[:, :2], dim=-1, keepdim=True), torch.zeros(total.shape[0], 1))
    assert torch.equal(g_on.xyz_gradient_accum, want) and want.max() > 1
    assert not torch.equal(g_off.xyz_gradient_accum, want)
    # only the statistics changed: loss and parameters are the flag-off step's; flag off is the step that never
    # heard of the option, bit for bit
    assert torch.equal(l_on, l_off) and torch.equal(l_off, l_none)
    for k in p_none:
        assert torch.equal(p_on[k], p_off[k]) and torch.equal(p_off[k], p_none[k]), k
    assert torch.equal(g_off.xyz_gradient_accum, g_none.xyz_gradient_accum)
    # a render_fn that leaves no .absgrad is an error with the option's name in it
    with pytest.raises(RuntimeError, match="densify_absgrad"):
        _step(views, _Renderer(forget=True), densify_absgrad=True)
