"""GPU tests of the opt-in absolute screen-space gradient (gs4d_backward_absgrad and everything above it).

Reference: tests/absgrad_refs.py, the fp64 restatement with one NDC-offset leaf per (pixel, list slot), on the 18
scenes of tests/depth_scenes.py, where no blend decision is near a threshold (tests/test_depth_grad_boundary.py
asserts it), so every element of every scene is compared.

The bar is the one tests/test_depth_grad_gpu.py uses for dL_dmeans2D on these scenes, |gpu - ref| <= GRAD_RTOL |ref|
+ F max|ref| with F = max(GRAD_FLOOR, 2 F0) from that module's `bars` fixture (F0 measured on the colour-only
backward); it is not chosen anew here.  absgrad's sums have the signed gradient's terms with the signs dropped, so
the same per-term rounding applies and nothing cancels.
"""
import numpy as np
import pytest
import torch

import absgrad_refs as AR
import depth_scenes as DS
import test_depth_grad_gpu as TD
from gpu_helpers import c_backward, c_forward, to_dev
from gs4d_train.synthetic import make_scene
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

bars = TD.bars  # the module-scoped fixture (F0, F) of tests/test_depth_grad_gpu.py
NAMES8 = PAR.GRAD_NAMES


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _dev(a):
    return torch.empty(0, device="cuda:0") if a is None else torch.tensor(a, device="cuda:0")


def _call(entry, s, d, fwd, grads, colors=None, cov3D=None, use_sh=True):
    """_C.<entry> with rasterize_gaussians_backward's arguments and `grads` (g_c, then g_d / g_a where the entry
    takes them; an empty tensor for "none") after the camera"""
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = fwd
    return getattr(_C(), entry)(
        d["bg"], d["means3D"], radii, e if colors is None else colors, e if cov3D is not None else d["scales"],
        e if cov3D is not None else d["rotations"], float(s["scale_modifier"]), e if cov3D is None else cov3D,
        d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), *grads,
        d["shs"] if use_sh else e, int(s["sh_degree"]), d["campos"], gb, nr, bb, ib, False)


def _scene_call(entry, name, *grads):
    sc, g = DS.scene(name), TD.gpu_forward(name)
    return _call(entry, sc["s"], g["d"], g["fwd"], [_dev(x) for x in grads], colors=g["colors"], cov3D=g["cov3D"],
                 use_sh=sc["use_sh"])


def backward_abs(name, g_c, g_d=None, g_a=None):
    """the 8 ordinary gradients and absgrad (P, 3)"""
    out = _scene_call("rasterize_gaussians_backward_absgrad", name, g_c, g_d, g_a)
    assert len(out) == 9 and tuple(out[8].shape) == tuple(out[0].shape)
    return out[:8], out[8]


def _fraction(a, ref, F):
    """the largest |a - ref| / (GRAD_RTOL |ref| + F max|ref|) over the elements"""
    scale = max(float(np.abs(ref).max()), 1e-30)
    return float((np.abs(a - ref) / (PAR.GRAD_RTOL * np.abs(ref) + F * scale)).max())


@pytest.mark.parametrize("case", ["color", "both", "sign"])
@pytest.mark.parametrize("name", DS.NAMES)
def test_absgrad_matches_fp64_and_dominates_the_signed_gradient(oracle, bars, name, case):
    """Parity: every element of absgrad against the fp64 reference, within the dL_dmeans2D bar of these scenes.
    Dominance: |means2D.grad| <= absgrad elementwise within the same bar; column 2 exactly 0; culled rows exactly 0.
    "color" runs the colour-only absgrad walk, "both" and "sign" the one with the depth gradient."""
    f0, F = bars
    g_c, g_d = DS.upstream(name, case)
    radii = TD.gpu_forward(name)["fwd"][3].cpu().numpy()
    assert np.array_equal(radii, DS.reference(oracle, name)["radii"])
    ref = AR.scene_absgrad(oracle, name, g_c, g_d)
    grads, absg = backward_abs(name, g_c, None if case == "color" else g_d)
    absg = absg.cpu().numpy().astype(np.float64)
    assert np.isfinite(absg).all() and not np.any(absg[:, 2]) and not np.any(absg[radii == 0])
    assert np.all(absg >= 0) and ref.max() > 0
    frac = _fraction(absg[:, :2], ref, F)
    signed = np.abs(grads[0].cpu().numpy().astype(np.float64)[:, :2])
    bar = PAR.GRAD_RTOL * np.abs(ref) + F * float(ref.max())
    over = float(((signed - absg[:, :2]) / bar).max())
    print(f"[absgrad-bars] {name} {case}: parity uses {frac:.3f} of the bar (F = {F:.3e}), dominance "
          f"{max(over, 0.0):.3f}; sum |grad| / sum absgrad = {signed.sum() / absg.sum():.3f}", flush=True)
    assert frac <= 1.0, f"absgrad: an element off by {frac:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"
    assert over <= 1.0, f"|means2D.grad| exceeds absgrad by {over:.2f}x the bar"


@pytest.mark.parametrize("name", DS.NAMES)
def test_absgrad_moves_nothing_else(name):
    """with absgrad on, every ordinary gradient is the absgrad-off call's bit for bit, in all four depth x alpha
    combinations"""
    g_c, g_d = DS.upstream(name, "both")
    g_a = np.random.default_rng(7).normal(0, 1, g_d.shape).astype(np.float32)
    for dep, alp in ((None, None), (g_d, None), (None, g_a), (g_d, g_a)):
        if dep is None and alp is None:
            off = _scene_call("rasterize_gaussians_backward", name, g_c)
        elif alp is None:
            off = _scene_call("rasterize_gaussians_backward_depth", name, g_c, dep)
        else:
            off = _scene_call("rasterize_gaussians_backward_aux", name, g_c, dep, alp)
        on, absg = backward_abs(name, g_c, dep, alp)
        for n, x, y in zip(NAMES8, on, off):
            assert x.shape == y.shape and torch.equal(x, y), (n, dep is not None, alp is not None)
        assert absg[:, :2].abs().max() > 0


@pytest.mark.parametrize("name", [n for n in DS.NAMES if n.startswith("dense")] + ["hi2"])
def test_absgrad_is_bitwise_repeatable(name):
    g_c, g_d = DS.upstream(name, "both")
    for dep in (None, g_d):
        a, b = backward_abs(name, g_c, dep)[1], backward_abs(name, g_c, dep)[1]
        assert torch.equal(a, b) and a.abs().max() > 0


# ---- known answers, through the autograd surface ----
def _settings(s, d):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=1.0, viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"], sh_degree=3, campos=d["campos"],
        prefiltered=False, debug=False)


def _raster(s, d, **kw):
    import diff_gaussian_rasterization as dgr
    L = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=True)
    out = dgr.GaussianRasterizer(_settings(s, d), **kw)(
        means3D=L["means3D"], means2D=L["means2D"], shs=L["shs"], opacities=L["opacities"], scales=L["scales"],
        rotations=L["rotations"])
    return L, out


def _one_gaussian():
    """one isotropic Gaussian on the optical axis of a 32 x 32 image: its centre projects to (15.5, 15.5), the
    corner shared by four pixels and four tiles, so its footprint is mirror-symmetric in x and in y"""
    s = make_scene(1, 32, 32, seed=0)
    s["means3D"] = np.array([[0.0, 0.0, 4.0]], np.float32)
    s["scales"] = np.full((1, 3), 0.3, np.float32)
    s["rotations"] = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    s["opacities"] = np.full((1, 1), 0.6, np.float32)
    s["shs"] = np.zeros((1, 16, 3), np.float32)
    s["shs"][:, 0, :] = -1.0  # colour 0.5 - 0.28 = 0.22 on the white background
    return s, to_dev(s, torch.device("cuda:0"))


def test_known_answer_symmetric_pull_cancels_in_grad_and_not_in_absgrad(bars):
    f0, F = bars
    s, d = _one_gaussian()
    # a constant positive upstream: every pixel's pull is mirrored by another pixel's
    L, (color, radii, depth) = _raster(s, d, absgrad=True)
    assert int(radii[0]) > 4
    color.backward(torch.ones_like(color))
    grad, absg = L["means2D"].grad, L["means2D"].absgrad
    assert tuple(absg.shape) == (1, 3) and float(absg[0, 2]) == 0.0
    assert (absg[0, :2] > 0).all()
    assert (grad[0, :2].abs() < 1e-3 * absg[0, :2]).all(), (grad, absg)
    # upstream at one pixel only: one term, so its absolute value is the absolute value of the sum
    L, (color, radii, depth) = _raster(s, d, absgrad=True)
    g = torch.zeros_like(color)
    g[:, 13, 17] = 1.0
    color.backward(g)
    grad, absg = L["means2D"].grad[0, :2].abs().cpu().numpy(), L["means2D"].absgrad[0, :2].cpu().numpy()
    assert grad.min() > 0
    assert _fraction(absg.astype(np.float64), grad.astype(np.float64), F) <= 1.0, (grad, absg)


def test_autograd_surface_composes_and_overwrites(oracle):
    """means2D.absgrad is the _C entry's tensor in every depth x alpha combination, the ordinary .grad values are
    the absgrad=False Functions', absgrad is overwritten per backward call, and the default leaves no attribute"""
    name = "rot1"
    s, d = DS.scene(name)["s"], TD.gpu_forward(name)["d"]
    g_c, g_d = (torch.tensor(x, device="cuda:0") for x in DS.upstream(name, "both"))
    g_a = torch.tensor(np.random.default_rng(7).normal(0, 1, tuple(g_d.shape)).astype(np.float32), device="cuda:0")
    for depth_grad in (False, True):
        for alpha in (False, True):
            res = {}
            for absgrad in (False, True):
                kw = dict(depth_grad=depth_grad, alpha=alpha)
                L, out = _raster(s, d, **kw, **({"absgrad": True} if absgrad else {}))
                loss = (out[0] * g_c).sum() + (out[2] * g_d).sum()  # the depth term is dropped without depth_grad
                if alpha:
                    loss = loss + (out[3] * g_a).sum()
                loss.backward()
                res[absgrad] = L
            on, off = res[True], res[False]
            for k in off:
                assert torch.equal(on[k].grad, off[k].grad), (k, depth_grad, alpha)
            assert not hasattr(off["means2D"], "absgrad")
            want = backward_abs(name, g_c.cpu().numpy(), g_d.cpu().numpy() if depth_grad else None,
                                g_a.cpu().numpy() if alpha else None)[1]
            assert torch.equal(on["means2D"].absgrad, want), (depth_grad, alpha)
    # overwritten, not accumulated: a second backward through a retained graph with twice the upstream
    L, out = _raster(s, d, absgrad=True)
    (out[0] * g_c).sum().backward(retain_graph=True)
    first = L["means2D"].absgrad.clone()
    (out[0] * (2 * g_c)).sum().backward()
    assert torch.equal(L["means2D"].absgrad, 2 * first)  # a power of two scales every term exactly


def test_autograd_matrix_is_the_direct_entries_tuple():
    """Every (depth_grad, alpha, absgrad) Function, with the loss built from the colour image only, the depth image
    only, the alpha image only (where there is one) and all of them: each leaf's .grad is, bit for bit, the tensor
    of the direct _C entry the Function stands for, called on the same scene's forward buffers with zeros / empty
    tensors for what the loss did not use; where nothing can flow (only the depth image used without depth_grad)
    every leaf stays without .grad and means2D without .absgrad.  small0: P = 60, 70 x 45 (partial tiles)."""
    name = "small0"
    sc, g = DS.scene(name), TD.gpu_forward(name)
    s, d = sc["s"], g["d"]
    gen = torch.Generator().manual_seed(11)
    g_c, g_d, g_a = (torch.randn(c, s["H"], s["W"], generator=gen).to("cuda:0") for c in (3, 1, 1))
    e = torch.empty(0, device="cuda:0")
    # position of each leaf's gradient in the entries' tuple
    slot = {"means3D": 3, "means2D": 0, "shs": 5, "opacities": 2, "scales": 6, "rotations": 7}

    def direct(entry, *grads):
        return _call(entry, s, d, g["fwd"], list(grads), colors=g["colors"], cov3D=g["cov3D"], use_sh=sc["use_sh"])

    for absgrad in (False, True):
        for alpha in (False, True):
            for depth_grad in (False, True):
                every = ("c", "d", "a") if alpha else ("c", "d")
                for use in [("c",), ("d",)] + ([("a",)] if alpha else []) + [every]:
                    what = (depth_grad, alpha, absgrad, use)
                    L, out = _raster(s, d, depth_grad=depth_grad, alpha=alpha, absgrad=absgrad)
                    assert len(out) == (4 if alpha else 3)
                    up = {"c": (0, g_c), "d": (2, g_d), "a": (3, g_a)}
                    sum((out[up[k][0]] * up[k][1]).sum() for k in use).backward()
                    gc = g_c if "c" in use else None
                    gd = g_d if "d" in use and depth_grad else None  # dropped unless depth_grad is set
                    ga = g_a if "a" in use else None
                    if gc is None and gd is None and ga is None:
                        assert all(t.grad is None for t in L.values()), what
                        assert not hasattr(L["means2D"], "absgrad"), what
                        continue
                    if alpha or absgrad:  # a missing colour gradient is zeros, a missing depth / alpha one is empty
                        want = direct("rasterize_gaussians_backward_absgrad" if absgrad
                                      else "rasterize_gaussians_backward_aux",
                                      torch.zeros_like(g_c) if gc is None else gc, e if gd is None else gd,
                                      e if ga is None else ga)
                    elif depth_grad:  # both as zeros
                        want = direct("rasterize_gaussians_backward_depth",
                                      torch.zeros_like(g_c) if gc is None else gc,
                                      torch.zeros_like(g_d) if gd is None else gd)
                    else:
                        want = direct("rasterize_gaussians_backward", gc)
                    assert len(want) == (9 if absgrad else 8)
                    for k, t in L.items():
                        assert t.grad is not None and torch.equal(t.grad, want[slot[k]]), (k, what)
                    assert want[0].abs().max() > 0
                    if absgrad:
                        assert torch.equal(L["means2D"].absgrad, want[8]) and want[8].abs().max() > 0, what
                    else:
                        assert not hasattr(L["means2D"], "absgrad"), what


# ---- edges ----
def test_empty_culled_and_partly_culled_scenes():
    dev = torch.device("cuda:0")
    # P = 0, through the Python surface
    s = make_scene(100, 64, 48, seed=14)
    s0 = dict(s)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        s0[k] = s[k][:0]
    d0 = to_dev(s0, dev)
    e = torch.empty(0, device=dev)
    out = _call("rasterize_gaussians_backward_absgrad", s0, d0, c_forward(_C(), s0, d0),
                [torch.ones(3, 48, 64, device=dev), e, e])
    assert len(out) == 9 and tuple(out[8].shape) == (0, 3) and tuple(out[0].shape) == (0, 3)
    # some Gaussians behind the near plane: their rows are exact zeros, the others' are not all zero
    s1 = make_scene(100, 64, 48, seed=14)
    s1["means3D"][::3, 2] = 0.1
    d1 = to_dev(s1, dev)
    fwd = c_forward(_C(), s1, d1)
    g = torch.ones(3, 48, 64, device=dev)
    e = torch.empty(0, device=dev)
    out = _call("rasterize_gaussians_backward_absgrad", s1, d1, fwd, [g, e, e])
    radii = fwd[3]
    assert int((radii == 0).sum()) >= 34 and int((radii > 0).sum()) > 0
    assert not out[8][radii == 0].any() and out[8][radii > 0][:, :2].max() > 0 and not out[8][:, 2].any()
    for n, x, y in zip(NAMES8, out[:8], c_backward(_C(), s1, d1, fwd, g)):
        assert torch.equal(x, y), n
    # every Gaussian culled: not one instance, exact zeros everywhere
    s2 = make_scene(100, 64, 48, seed=14)
    s2["means3D"][:, 2] = 0.1
    d2 = to_dev(s2, dev)
    fwd = c_forward(_C(), s2, d2)
    assert fwd[0] == 0
    out = _call("rasterize_gaussians_backward_absgrad", s2, d2, fwd, [g, e, e])
    assert tuple(out[8].shape) == (100, 3) and not out[8].any()


# ---- train step ----
def _model(pts, cols, opt, hyper):
    return TD._train_model(pts, cols, opt, hyper)


def _params(g):
    out = {n: p.detach().clone() for n, p in g._deformation.named_parameters()}
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        out[name] = getattr(g, name).detach().clone()
    return out


def test_train_step_densifies_on_absgrad():
    """500 points, 64 x 48, two views, the fused step.  With densify_absgrad the statistics accumulate the norm of the
    views' summed .absgrad[:, :2] on the rows some view saw (radii > 0) and nothing elsewhere; the fused statistics
    kernel and torch.norm may round the two-element norm differently, so 4 ulp (5e-7 relative) is allowed.  With the
    flag False the step is, bit for bit, the step of options that never had the attribute."""
    from gs4d_train import config
    from gs4d_train.render import render
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    W, H, P = 64, 48, 500
    pts, cols = make_point_cloud(P, seed=5)
    views = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")

    def run(flag):
        hyper, opt = config.dynerf()
        if flag is None:
            del opt.densify_absgrad
        else:
            opt.densify_absgrad = flag
        g = _model(pts, cols, opt, hyper)
        pkgs = []

        def render_fn(*a, **kw):
            pkgs.append((render(*a, **kw), dict(kw)))
            return pkgs[-1][0]
        loss = train_step(g, views, opt, hyper, 3001, bg, render_fn=render_fn)
        return g, pkgs, loss

    g, pkgs, _ = run(True)
    assert [kw.get("absgrad") for _, kw in pkgs] == [True, True]
    total = pkgs[0][0]["viewspace_points"].absgrad + pkgs[1][0]["viewspace_points"].absgrad
    seen = (pkgs[0][0]["radii"] > 0) | (pkgs[1][0]["radii"] > 0)
    assert int(seen.sum()) > 100
    want = torch.where(seen, torch.norm(total[:, :2], dim=-1), torch.zeros_like(total[:, 0]))
    got = g.xyz_gradient_accum[:, 0]
    assert not got[~seen].any() and want[seen].min() > 0
    assert ((got - want).abs() <= 5e-7 * want).all()
    signed = pkgs[0][0]["viewspace_points"].grad + pkgs[1][0]["viewspace_points"].grad
    assert (want >= torch.norm(signed[:, :2], dim=-1) * (1 - 1e-3)).all() and want.sum() > signed[:, :2].norm(
        dim=-1).sum()

    g_off, pkgs_off, l_off = run(False)
    g_none, pkgs_none, l_none = run(None)
    assert all("absgrad" not in kw for _, kw in pkgs_off + pkgs_none)
    assert torch.equal(l_off, l_none)
    a, b = _params(g_off), _params(g_none)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(g_off.xyz_gradient_accum, g_none.xyz_gradient_accum)
    assert not hasattr(pkgs_off[0][0]["viewspace_points"], "absgrad")
