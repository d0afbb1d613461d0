"""GPU tests of the opt-in depth gradient (gs4d_backward_depth and everything above it).

Reference: the fp64 autograd restatement (tests/torch_restatement.py) of sum(color * g_c) + sum(depth * g_d) on
the scenes of tests/depth_scenes.py, where no discrete rule of the blend is near its threshold
(tests/test_depth_grad_boundary.py asserts it), so every element of every gradient tensor is compared.

The bar: |gpu - ref| <= GRAD_RTOL |ref| + F max|ref| per element (the form of oracle/parity.py).  F0 is the
smallest floor at which the existing colour-only backward meets that form against the colour-only autograd
gradient on these same scenes (measured here, by the `bars` fixture); F = max(GRAD_FLOOR, 2 F0): the depth term
adds one more rounded term to each sum, and its operand (a view depth of 2-6) is larger than a colour's.
"""
import numpy as np
import pytest
import torch

import depth_scenes as DS
from gpu_helpers import c_backward, c_forward, to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

NAMES8 = PAR.GRAD_NAMES
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def gpu_forward(name):
    """device tensors and the HIP forward of a scene, made once"""
    if name not in _GPU:
        sc = DS.scene(name)
        dev = torch.device("cuda:0")
        d = to_dev(sc["s"], dev)
        colors = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
        cov3D = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
        fwd = c_forward(_C(), sc["s"], d, colors=colors, cov3D=cov3D, use_sh=sc["use_sh"])
        _GPU[name] = dict(d=d, colors=colors, cov3D=cov3D, fwd=fwd)
    return _GPU[name]


def backward_color(name, g_c):
    sc, g = DS.scene(name), gpu_forward(name)
    return c_backward(_C(), sc["s"], g["d"], g["fwd"], torch.tensor(g_c, device="cuda:0"), colors=g["colors"],
                      cov3D=g["cov3D"], use_sh=sc["use_sh"])


def backward_depth(name, g_c, g_d):
    sc, g = DS.scene(name), gpu_forward(name)
    s, d = sc["s"], g["d"]
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = g["fwd"]
    cov = g["cov3D"]
    return _C().rasterize_gaussians_backward_depth(
        d["bg"], d["means3D"], radii, e if g["colors"] is None else g["colors"], e if cov is not None else d["scales"],
        e if cov is not None else d["rotations"], float(s["scale_modifier"]), e if cov is None else cov,
        d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), torch.tensor(g_c, device="cuda:0"),
        torch.tensor(g_d, device="cuda:0"), d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], gb, nr,
        bb, ib, False)


def _pairs(name, got, want):
    """(tensor name, gpu array, fp64 reference) of the gradients the scene's input mode has; dL_dmeans2D's third
    column and every row of a culled Gaussian must be exactly zero"""
    radii = gpu_forward(name)["fwd"][3].cpu().numpy()
    out = []
    for n, a, b in zip(NAMES8, got, want):
        a = a.detach().cpu().numpy()
        if n == "dL_dmeans2D":
            assert not np.any(a[:, 2])
            a = a[:, :2]
        assert np.isfinite(a).all(), n
        assert not np.any(a.reshape(len(radii), -1)[radii == 0]) if a.size else True, f"{n}: culled rows not zero"
        if b is None or a.size == 0:
            continue
        out.append((n, a.astype(np.float64).reshape(b.shape), np.asarray(b, np.float64)))
    return out


def needed_floor(pairs):
    """the smallest F with |a - b| <= GRAD_RTOL |b| + F max|b| for every element of every tensor"""
    f = 0.0
    for _, a, b in pairs:
        scale = max(float(np.abs(b).max()), 1e-30)
        f = max(f, float(np.maximum(np.abs(a - b) - PAR.GRAD_RTOL * np.abs(b), 0.0).max()) / scale)
    return f


@pytest.fixture(scope="module")
def bars(oracle):
    f0 = 0.0
    for name in DS.NAMES:
        g_c, g_d = DS.upstream(name, "color")
        want = DS.autograd_grads(oracle, name, g_c, g_d)
        f0 = max(f0, needed_floor(_pairs(name, backward_color(name, g_c), want)))
    F = max(PAR.GRAD_FLOOR, 2.0 * f0)
    print(f"[depth-bars] F0 = {f0:.3e} (colour-only backward against colour-only autograd), F = {F:.3e}", flush=True)
    return f0, F


@pytest.mark.parametrize("name", DS.NAMES)
def test_zero_depth_gradient_is_the_colour_backward_bitwise(oracle, name):
    g_c, g_d = DS.upstream(name, "both")
    a = backward_depth(name, g_c, np.zeros_like(g_d))
    b = backward_color(name, g_c)
    for n, x, y in zip(NAMES8, a, b):
        assert x.shape == y.shape and torch.equal(x, y), n


@pytest.mark.parametrize("case", ["depth", "both", "sign"])
@pytest.mark.parametrize("name", DS.NAMES)
def test_depth_gradient_matches_fp64_autograd(oracle, bars, name, case):
    f0, F = bars
    g_c, g_d = DS.upstream(name, case)
    assert np.array_equal(gpu_forward(name)["fwd"][3].cpu().numpy(), DS.reference(oracle, name)["radii"])
    pairs = _pairs(name, backward_depth(name, g_c, g_d), DS.autograd_grads(oracle, name, g_c, g_d))
    assert [n for n, _, _ in pairs][:4] == NAMES8[:4]
    worst = {}
    for n, a, b in pairs:
        scale = max(float(np.abs(b).max()), 1e-30)
        ratio = np.abs(a - b) / (PAR.GRAD_RTOL * np.abs(b) + F * scale)
        worst[n] = float(ratio.max())
    print(f"[depth-parity] {name} {case}: needs floor {needed_floor(pairs):.3e} of F = {F:.3e}; worst ratios "
          + " ".join(f"{n}={v:.3f}" for n, v in worst.items()), flush=True)
    for n, v in worst.items():
        assert v <= 1.0, f"{n}: an element off by {v:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"


def _leaves(name):
    g = gpu_forward(name)
    d = g["d"]
    L = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=True)
    return L


def _raster(name, L, depth_grad=None):
    import diff_gaussian_rasterization as dgr
    s, d = DS.scene(name)["s"], gpu_forward(name)["d"]
    st = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=1.0, viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"], sh_degree=3, campos=d["campos"],
        prefiltered=False, debug=False)
    r = dgr.GaussianRasterizer(st) if depth_grad is None else dgr.GaussianRasterizer(st, depth_grad=depth_grad)
    return r(means3D=L["means3D"], means2D=L["means2D"], shs=L["shs"], opacities=L["opacities"], scales=L["scales"],
             rotations=L["rotations"])


def test_autograd_surface(oracle):
    name = "rot1"
    # depth alone: gradients flow only under the opt-in
    L = _leaves(name)
    color, radii, depth = _raster(name, L, depth_grad=True)
    depth.sum().backward()
    assert L["means3D"].grad.abs().max() > 0 and L["opacities"].grad.abs().max() > 0
    assert L["shs"].grad is None or not L["shs"].grad.any()  # the depth image does not depend on the colours
    want = DS.autograd_grads(oracle, name, np.zeros((3,) + tuple(depth.shape[1:]), np.float32),
                             np.ones(tuple(depth.shape), np.float32))
    scale = np.abs(want[3]).max()
    assert np.abs(L["means3D"].grad.cpu().numpy() - want[3]).max() <= 1e-3 * scale
    L0 = _leaves(name)
    color0, _, depth0 = _raster(name, L0)
    assert torch.equal(depth0, depth) and torch.equal(color0, color)
    if depth0.requires_grad:
        depth0.sum().backward()
    for k in ("means3D", "opacities"):
        assert L0[k].grad is None or not L0[k].grad.any()
    # colour alone: the opt-in path gives the default path's gradients bit for bit
    g_c = torch.tensor(DS.upstream(name, "both")[0], device="cuda:0")
    La, Lb = _leaves(name), _leaves(name)
    (_raster(name, La, depth_grad=True)[0] * g_c).sum().backward()
    (_raster(name, Lb)[0] * g_c).sum().backward()
    for k in La:
        assert torch.equal(La[k].grad, Lb[k].grad), k


@pytest.mark.parametrize("name", [n for n in DS.NAMES if n.startswith("dense")])
def test_depth_backward_is_bitwise_repeatable(name):
    g_c, g_d = DS.upstream(name, "both")
    a = backward_depth(name, g_c, g_d)
    b = backward_depth(name, g_c, g_d)
    for n, x, y in zip(NAMES8, a, b):
        assert torch.equal(x, y), n
    assert a[3].abs().max() > 0


def _train_model(pts, cols, opt, hyper):
    from gs4d_train.gaussians import GaussianModel
    torch.manual_seed(7)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = True  # the bitwise-repeatable step (test_train_step_deterministic)
    g._deformation.deformation_net.fused_heads = True
    g.training_setup(opt)
    g.active_sh_degree = 3
    return g


def _step_grads(pts, cols, views, opt, hyper, **kw):
    from gs4d_train.train import train_step
    g = _train_model(pts, cols, opt, hyper)
    loss = train_step(g, views, opt, hyper, 3001, torch.ones(3, device="cuda"), **kw)
    grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        grads[name] = getattr(g, name).grad.detach().clone()
    return float(loss), grads, g


def test_train_step_with_depth_loss():
    """One fine-stage step with lambda_depth = 0.5 on (camera, gt, gt_depth) views, the fused loss (explicit colour
    and depth gradients, one autograd.backward) against the unfused one (torch autograd through the loss), with
    the bars of test_train_gpu.py::test_train_step_fused_matches_torch_tail: the optimizer is held back so the
    parameter gradients themselves are compared, 1e-3 of each tensor's max and 1e-4 at the 99.9th percentile,
    the loss within 1e-5.  Then lambda_depth = 0 with the same triple views is the pair-view step bit for bit."""
    from gs4d_train import config
    from gs4d_train.render import render
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    W, H, P = 64, 48, 3000
    hyper, opt = config.dynerf()
    opt.iterations = 0
    pts, cols = make_point_cloud(P, seed=5)
    pairs = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")
    # ground-truth depth: the render of a perturbed copy of the model (0 = nothing there: invalid)
    moved = (pts + np.random.default_rng(8).normal(0, 0.05, pts.shape)).astype(np.float32)
    other = _train_model(moved, cols, opt, hyper)
    with torch.no_grad():
        triples = [(cam, gt, render(cam, other, False, bg)["depth"].clone()) for cam, gt in pairs]
    assert all(((d > 0).float().mean() > 0.2) for _, _, d in triples)
    triples[1] = (triples[1][0], triples[1][1], triples[1][2][0])  # (H, W) is accepted as well

    opt.lambda_depth = 0.5
    lf, gf, _ = _step_grads(pts, cols, triples, opt, hyper, fused_loss=True)
    lu, gu, _ = _step_grads(pts, cols, triples, opt, hyper, fused_loss=False)
    l0, g0, _ = _step_grads(pts, cols, pairs, opt, hyper, fused_loss=True)
    assert abs(lf - lu) <= 1e-5 * abs(lu)
    assert lf > l0 and gf.keys() == gu.keys()
    assert not torch.equal(gf["_xyz"], g0["_xyz"])  # the depth term reached the Gaussians
    for k in gu:
        a, b = gu[k], gf[k]
        scale = max(a.abs().max().item(), 1e-30)
        d = (a - b).abs().flatten() / scale
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k

    opt.lambda_depth = 0.0
    for fused in (True, False):
        lt, gt_, _ = _step_grads(pts, cols, triples, opt, hyper, fused_loss=fused)
        lp, gp, _ = _step_grads(pts, cols, pairs, opt, hyper, fused_loss=fused)
        assert lt == lp and gt_.keys() == gp.keys()
        for k in gp:
            assert torch.equal(gt_[k], gp[k]), k
