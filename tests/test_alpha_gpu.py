"""GPU tests of the opt-in alpha image (gs4d_alpha_image, gs4d_backward_aux, gs4d_aux_loss_grad and everything
above them).

Reference for values and gradients: the fp64 autograd restatement (tests/torch_restatement.py), whose Tfinal is
differentiable, on the scenes of tests/depth_scenes.py, where no discrete rule of the blend is near its threshold
(tests/test_depth_grad_boundary.py asserts it), so every element is compared.  The scenes of tests/alpha_scenes.py,
where termination, the 0.99 cap and the 1/255 rule do bite, are checked by identities between the GPU's own results.

The gradient bar is test_depth_grad_gpu.py's: |gpu - ref| <= GRAD_RTOL |ref| + F max|ref| per element, with
F = max(GRAD_FLOOR, 2 F0) and F0 the smallest floor at which the existing colour-only backward meets that form on
these scenes (measured here).  The alpha term adds one rounded operand of magnitude <= |g_A| to the start value of
the walk's running sum, no more than the depth term that rule was set for.
"""
import numpy as np
import pytest
import torch

import alpha_scenes as AS
import depth_scenes as DS
from gpu_helpers import c_backward, c_forward, to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

NAMES8 = PAR.GRAD_NAMES
IDENTITY_SCENES = ["opaque"] + [n for n in DS.NAMES if n.startswith(("dense", "hi"))]
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _scene(name):
    return AS.scene(name) if name in AS.NAMES else DS.scene(name)


def gpu_forward(name, bg=None):
    """device tensors and the HIP forward of a scene (with the scene's background, or `bg` for all channels), made
    once"""
    key = (name, bg)
    if key not in _GPU:
        sc = _scene(name)
        dev = torch.device("cuda:0")
        d = to_dev(sc["s"], dev)
        if bg is not None:
            d["bg"] = torch.full((3,), float(bg), device=dev)
        colors = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
        cov3D = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
        fwd = c_forward(_C(), sc["s"], d, colors=colors, cov3D=cov3D, use_sh=sc["use_sh"])
        s = sc["s"]
        alpha = _C().alpha_image(fwd[6], int(s["H"]), int(s["W"]))
        _GPU[key] = dict(d=d, colors=colors, cov3D=cov3D, fwd=fwd, alpha=alpha)
    return _GPU[key]


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _backward(entry, name, grads, bg=None):
    """a _C backward entry with the scene's tensors; grads = the gradient images in the entry's order (None = the
    empty tensor, "no such gradient"); bg = another background vector for this call"""
    sc, g = _scene(name), gpu_forward(name)
    s, d = sc["s"], g["d"]
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = g["fwd"]
    cov = g["cov3D"]
    imgs = [e if x is None else _dev(x) for x in grads]
    return getattr(_C(), entry)(
        d["bg"] if bg is None else _dev(np.asarray(bg, np.float32)), d["means3D"], radii,
        e if g["colors"] is None else g["colors"], e if cov is not None else d["scales"],
        e if cov is not None else d["rotations"], float(s["scale_modifier"]), e if cov is None else cov,
        d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), *imgs,
        d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], gb, nr, bb, ib, False)


def backward_color(name, g_c, bg=None):
    return _backward("rasterize_gaussians_backward", name, [g_c], bg)


def backward_depth(name, g_c, g_d, bg=None):
    return _backward("rasterize_gaussians_backward_depth", name, [g_c, g_d], bg)


def backward_aux(name, g_c, g_d, g_a, bg=None):
    return _backward("rasterize_gaussians_backward_aux", name, [g_c, g_d, g_a], bg)


def _same(a, b):
    for n, x, y in zip(NAMES8, a, b):
        assert x.shape == y.shape and torch.equal(x, y), n


def _upstream(name, case):
    """(g_c, g_d, g_A) float32: "alpha" g_A ~ N(0, 1) alone; "all" depth_scenes' "both" with the same g_A; "sign" a
    +-1 pattern for g_A alone"""
    s = _scene(name)["s"]
    H, W = s["H"], s["W"]
    seed = DS.ENTRIES[DS.NAMES.index(name)]["seed"] if name in DS.NAMES else 0
    rng = np.random.default_rng(2000 + seed)
    g_a = rng.normal(0, 1, (1, H, W)).astype(np.float32)
    g_c, g_d = np.zeros((3, H, W), np.float32), np.zeros((1, H, W), np.float32)
    if case == "all":
        g_c, g_d = DS.upstream(name, "both")
    elif case == "sign":
        g_a = np.where(rng.uniform(0, 1, (1, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
    else:
        assert case == "alpha"
    return g_c, g_d, g_a


def autograd_grads(O, name, g_c, g_d, g_a):
    """depth_scenes.autograd_grads with the alpha term: fp64 gradients of
    sum(color * g_c) + sum(depth * g_d) + sum((1 - Tfinal) * g_A)"""
    sc = DS.scene(name)
    ref = DS.reference(O, name)["ref"]
    leaves = [ref["ndc_off"], ref["rgb"], ref["opac"], ref["means"], ref["cov3"], ref["shs"], ref["scales"],
              ref["rots"]]
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    loss = (ref["color"] * f64(g_c)).sum() + (ref["depth"] * f64(g_d)).sum() + \
        ((1.0 - ref["Tfinal"]) * f64(g_a)[0]).sum()
    gr = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    z = lambda t, like: np.zeros(tuple(like.shape)) if t is None else t.numpy()
    dm2, dcol, dop, dm3, gc, dsh, dsc, drot = (z(g, l) for g, l in zip(gr, leaves))
    packed = np.stack([gc[:, 0, 0], gc[:, 0, 1] + gc[:, 1, 0], gc[:, 0, 2] + gc[:, 2, 0], gc[:, 1, 1],
                       gc[:, 1, 2] + gc[:, 2, 1], gc[:, 2, 2]], 1)
    return [dm2, dcol, dop, dm3, packed, dsh if sc["mode"] == "sh" else None,
            dsc if sc["mode"] != "cov3D" else None, drot if sc["mode"] != "cov3D" else None]


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
    print(f"[alpha-bars] F0 = {f0:.3e} (colour-only backward against colour-only autograd), F = {F:.3e}", flush=True)
    return f0, F


# ---- 1. value --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DS.NAMES)
def test_alpha_image_matches_fp64(oracle, name):
    r = DS.reference(oracle, name)
    alpha = gpu_forward(name)["alpha"]
    s = DS.scene(name)["s"]
    assert alpha.shape == (1, s["H"], s["W"]) and alpha.dtype == torch.float32
    a = alpha[0].cpu().numpy().astype(np.float64)
    want = 1.0 - r["ref"]["Tfinal"].detach().numpy()
    err = float(np.abs(a - want).max())
    print(f"[alpha-value] {name}: max |alpha - (1 - Tfinal)| = {err:.3e} (bar {PAR.IMG_ATOL})", flush=True)
    assert err <= PAR.IMG_ATOL
    assert not np.any(a[np.asarray(r["export"]["n_contrib"]).reshape(a.shape) == 0])
    assert a.min() >= 0.0 and a.max() < 1.0


def _leaves(name):
    d = gpu_forward(name)["d"]
    L = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=True)
    return L


def _raster(name, L, **kw):
    import diff_gaussian_rasterization as dgr
    s, d = _scene(name)["s"], gpu_forward(name)["d"]
    st = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=1.0, viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"], sh_degree=3, campos=d["campos"],
        prefiltered=False, debug=False)
    return dgr.GaussianRasterizer(st, **kw)(means3D=L["means3D"], means2D=L["means2D"], shs=L["shs"],
                                           opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"])


@pytest.mark.parametrize("name", ["small0", "dense1", "opaque", "sparse"])
def test_alpha_forward_leaves_the_other_outputs_alone(name):
    out = _raster(name, _leaves(name), alpha=True)
    ref = _raster(name, _leaves(name))
    assert len(out) == 4 and len(ref) == 3
    for x, y in zip(out[:3], ref):
        assert torch.equal(x, y)
    assert torch.equal(out[3], gpu_forward(name)["alpha"])
    both = _raster(name, _leaves(name), alpha=True, depth_grad=True)
    assert len(both) == 4 and all(torch.equal(x, y) for x, y in zip(both, out))


def test_alpha_is_zero_where_nothing_is_drawn(oracle):
    s = AS.scene("sparse")["s"]
    r = AS.reference(oracle, "sparse")
    a = gpu_forward("sparse")["alpha"][0].cpu().numpy()
    empty = AS.tile_is_empty(r, s["H"], s["W"])
    assert empty.sum() > 0 and not np.any(a[empty])
    assert not np.any(a[r["n_contrib"] == 0]) and a.max() > 0 and a.min() >= 0 and a.max() < 1
    assert np.abs(a - (1.0 - r["final_T"].astype(np.float64))).max() <= PAR.IMG_ATOL
    # every Gaussian behind the camera: P > 0, not one instance, and the image state still holds T = 1
    g = gpu_forward("behind")
    assert g["d"]["means3D"].shape[0] > 0 and g["fwd"][0] == 0
    assert g["alpha"].shape == (1, s["H"], s["W"]) and not g["alpha"].any()
    # no Gaussians at all: zeros from the Python layer, without an image state
    import diff_gaussian_rasterization as dgr
    d = g["d"]
    st = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=1.0, viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"], sh_degree=3, campos=d["campos"],
        prefiltered=False, debug=False)
    z = lambda *shape: torch.zeros(*shape, device="cuda:0")
    out = dgr.GaussianRasterizer(st, alpha=True)(means3D=z(0, 3), means2D=z(0, 3), shs=z(0, 16, 3),
                                                 opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    assert out[3].shape == (1, s["H"], s["W"]) and not out[3].any()


# ---- 2. consistency with the colour ----------------------------------------------------------------------------
def test_alpha_is_the_background_weight_of_the_colour():
    """color = C + T_final bg, so color(bg = 1) - color(bg = 0) = T_final = 1 - alpha in every channel: both
    forwards take identical blend decisions, and each side is a handful of fp32 roundings at magnitude <= 2"""
    c1 = gpu_forward("opaque", bg=1.0)["fwd"][1]
    c0 = gpu_forward("opaque", bg=0.0)["fwd"][1]
    alpha = gpu_forward("opaque", bg=0.0)["alpha"]
    assert torch.equal(alpha, gpu_forward("opaque", bg=1.0)["alpha"]) and torch.equal(alpha, gpu_forward("opaque")["alpha"])
    err = ((c1 - c0) - (1.0 - alpha)).abs().amax(dim=(1, 2))
    print(f"[alpha-colour] opaque: max |(color_bg1 - color_bg0) - (1 - alpha)| per channel = {err.tolist()}", flush=True)
    assert float(err.max()) <= 1e-6


# ---- 3. null alpha gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DS.NAMES)
def test_no_alpha_gradient_is_the_existing_backward_bitwise(oracle, name):
    g_c, g_d = DS.upstream(name, "both")
    _same(backward_aux(name, g_c, g_d, None), backward_depth(name, g_c, g_d))
    _same(backward_aux(name, g_c, None, None), backward_color(name, g_c))


# ---- 4. background-shift identity ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_alpha_gradient_is_a_background_shift_bitwise(oracle, name):
    """dL/dalpha enters as a0 = bg . dL/dpix - dL/dA.  With bg = 0 and g_A = -0.5 g_c[0] that is 0.5 d0 exactly, what
    bg = (0.5, 0, 0) gives without an alpha gradient (0.5 d0 + 0 + 0, exact with or without contraction): the same
    walk from the same start value, whatever rule bites along it."""
    s = _scene(name)["s"]
    if name in DS.NAMES:
        g_c, g_d = DS.upstream(name, "both")
    else:
        rng = np.random.default_rng(5)
        g_c = rng.normal(0, 1, (3, s["H"], s["W"])).astype(np.float32)
        g_d = rng.normal(0, 1, (1, s["H"], s["W"])).astype(np.float32)
    assert np.all(g_c[0] != 0)
    g_a = (-0.5 * g_c[0:1]).astype(np.float32)
    zero, half = [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]
    a = backward_aux(name, g_c, None, g_a, bg=zero)
    _same(a, backward_color(name, g_c, bg=half))
    _same(backward_aux(name, g_c, g_d, g_a, bg=zero), backward_depth(name, g_c, g_d, bg=half))
    assert not torch.equal(a[2], backward_color(name, g_c, bg=zero)[2])  # and the alpha gradient did something


# ---- 5. fp64 autograd parity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["alpha", "all", "sign"])
@pytest.mark.parametrize("name", DS.NAMES)
def test_alpha_gradient_matches_fp64_autograd(oracle, bars, name, case):
    f0, F = bars
    g_c, g_d, g_a = _upstream(name, case)
    assert np.array_equal(gpu_forward(name)["fwd"][3].cpu().numpy(), DS.reference(oracle, name)["radii"])
    # "alpha": the colour-only instantiation; "sign": the depth one with a zero depth gradient; "all": everything
    got = backward_aux(name, g_c, None if case == "alpha" else g_d, g_a)
    pairs = _pairs(name, got, autograd_grads(oracle, name, g_c, g_d, g_a))
    assert [n for n, _, _ in pairs][:4] == NAMES8[:4]
    worst = {}
    for n, a, b in pairs:
        scale = max(float(np.abs(b).max()), 1e-30)
        worst[n] = float((np.abs(a - b) / (PAR.GRAD_RTOL * np.abs(b) + F * scale)).max())
    print(f"[alpha-parity] {name} {case}: F0 = {f0:.3e}, needs floor {needed_floor(pairs):.3e} of F = {F:.3e}; "
          "worst ratios " + " ".join(f"{n}={v:.3f}" for n, v in worst.items()), flush=True)
    if case != "all":  # the alpha image does not depend on the colours
        assert not got[1].any() and not got[5].any()
    assert got[2].abs().max() > 0 and got[3].abs().max() > 0
    for n, v in worst.items():
        assert v <= 1.0, f"{n}: an element off by {v:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"


# ---- 6. repeatability ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in DS.NAMES if n.startswith("dense")] + ["opaque"])
def test_aux_backward_is_bitwise_repeatable(oracle, name):
    s = _scene(name)["s"]
    rng = np.random.default_rng(9)
    g_c = rng.normal(0, 1, (3, s["H"], s["W"])).astype(np.float32)
    g_d = rng.normal(0, 1, (1, s["H"], s["W"])).astype(np.float32)
    g_a = rng.normal(0, 1, (1, s["H"], s["W"])).astype(np.float32)
    for d in (g_d, None):
        a = backward_aux(name, g_c, d, g_a)
        _same(a, backward_aux(name, g_c, d, g_a))
        assert a[3].abs().max() > 0


# ---- 7. autograd surface ---------------------------------------------------------------------------------------
def test_autograd_surface(oracle):
    name = "rot1"
    # alpha alone
    L = _leaves(name)
    color, radii, depth, alpha = _raster(name, L, alpha=True)
    alpha.sum().backward()
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert L[k].grad is not None and L[k].grad.abs().max() > 0, k
    assert L["shs"].grad is None or not L["shs"].grad.any()
    # without depth_grad the depth image's gradient is dropped on the alpha path too
    L = _leaves(name)
    depth_only = _raster(name, L, alpha=True)[2]
    if depth_only.requires_grad:
        depth_only.sum().backward()
    assert L["means3D"].grad is None or not L["means3D"].grad.any()
    # normalised depth through both opt-ins against fp64 autograd of the same expression
    L = _leaves(name)
    color, radii, depth, alpha = _raster(name, L, depth_grad=True, alpha=True)
    (depth / alpha.clamp_min(0.05)).sum().backward()
    ref = DS.reference(oracle, name)["ref"]
    A = (1.0 - ref["Tfinal"]).reshape(ref["depth"].shape)
    want = torch.autograd.grad((ref["depth"] / A.clamp_min(0.05)).sum(), ref["means"], retain_graph=True)[0].numpy()
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(L["means3D"].grad.cpu().numpy() - want).max() <= 1e-3 * scale
    # colour alone: the alpha path gives the default path's gradients bit for bit
    g_c = torch.tensor(DS.upstream(name, "both")[0], device="cuda:0")
    La, Lb, Lc = _leaves(name), _leaves(name), _leaves(name)
    (_raster(name, La, alpha=True)[0] * g_c).sum().backward()
    (_raster(name, Lb)[0] * g_c).sum().backward()
    (_raster(name, Lc, alpha=True, depth_grad=True)[0] * g_c).sum().backward()
    for k in La:
        assert torch.equal(La[k].grad, Lb[k].grad) and torch.equal(Lc[k].grad, Lb[k].grad), k


# ---- 8. the fused loss -----------------------------------------------------------------------------------------
def _aux_inputs(shape):
    rng = np.random.default_rng(int(np.prod(shape)))
    depth = rng.uniform(0.0, 6.0, shape).astype(np.float32)
    gt_depth = (depth + rng.normal(0, 0.5, shape)).astype(np.float32)
    flat = gt_depth.reshape(-1)
    flat[rng.uniform(0, 1, flat.size) < 0.3] = 0.0      # invalid pixels
    flat[rng.uniform(0, 1, flat.size) < 0.05] = -1.0
    alpha = rng.uniform(0, 1, shape).astype(np.float32)
    gt_mask = (rng.uniform(0, 1, shape) < 0.5).astype(np.float32)
    n = flat.size
    if n > 8:  # planted ties on valid pixels
        gt_depth.reshape(-1)[2] = depth.reshape(-1)[2] = 3.25
        gt_mask.reshape(-1)[5] = alpha.reshape(-1)[5] = 1.0
        gt_mask.reshape(-1)[n - 1] = alpha.reshape(-1)[n - 1] = 0.0
    else:
        gt_depth.reshape(-1)[0] = 2.0
    return [torch.tensor(a, device="cuda:0") for a in (depth, alpha, gt_depth, gt_mask)]


def _aux_reference(depth, alpha, gt_depth, gt_mask, w_d, w_m):
    """the fp64 torch formulation (train.depth_l1's semantics): value, dL/ddepth, dL/dalpha"""
    f64 = lambda t: t.detach().double().cpu()
    value = torch.zeros((), dtype=torch.float64)
    g_d = g_a = None
    if gt_depth is not None:
        d, gd = f64(depth), f64(gt_depth)
        valid = gd > 0
        nv = valid.sum().clamp(min=1).double()
        diff = torch.where(valid, d - gd, torch.zeros_like(d))
        value = value + w_d * diff.abs().sum() / nv
        g_d = w_d * torch.sign(diff) / nv
    if gt_mask is not None:
        a, gm = f64(alpha), f64(gt_mask)
        value = value + w_m * (a - gm).abs().mean()
        g_a = w_m * torch.sign(a - gm) / a.numel()
    return value, g_d, g_a


@pytest.mark.parametrize("case", ["depth", "mask", "both", "invalid"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 3), (1, 45, 70)])
def test_aux_loss_and_grad_matches_fp64(shape, case):
    from gs4d_train.kernels import aux_loss_and_grad
    depth, alpha, gt_depth, gt_mask = _aux_inputs(shape)
    w_d, w_m = 0.7, 0.3
    if case == "invalid":  # gt_depth <= 0 everywhere: no valid pixel, n_valid = max(1, 0)
        gt_depth = -gt_depth.abs()
    use_d = None if case == "mask" else gt_depth
    use_m = None if case in ("depth", "invalid") else gt_mask
    value, g_d, g_a = aux_loss_and_grad(depth, alpha, use_d, use_m, w_d, w_m)
    value2, g_d2, g_a2 = aux_loss_and_grad(depth, alpha, use_d, use_m, w_d, w_m)
    want, r_d, r_a = _aux_reference(depth, alpha, use_d, use_m, w_d, w_m)
    assert value.shape == () and torch.equal(value, value2)
    print(f"[aux-loss] {shape} {case}: value {float(value):.7g} against {float(want):.7g}", flush=True)
    assert abs(float(value) - float(want)) <= 1e-5 * abs(float(want))
    for g, g2, r, like in ((g_d, g_d2, r_d, depth), (g_a, g_a2, r_a, alpha)):
        assert (g is None) == (r is None)
        if g is None:
            continue
        assert g.shape == like.shape and g.dtype == torch.float32 and torch.equal(g, g2)
        got = g.double().cpu()
        assert bool(((got - r).abs() <= 1e-6 * r.abs()).all())  # exactly 0 where the reference is 0
    if case == "invalid":
        assert float(value) == 0.0 and not g_d.any()
    n = int(np.prod(shape))
    if n > 8 and g_d is not None and case != "invalid":
        assert float(g_d.reshape(-1)[2]) == 0.0 and g_d.abs().max() > 0
        assert not g_d.reshape(-1)[(gt_depth <= 0).reshape(-1)].any()
    if n > 8 and g_a is not None:
        assert float(g_a.reshape(-1)[5]) == 0.0 and float(g_a.reshape(-1)[n - 1]) == 0.0 and g_a.abs().max() > 0


# ---- 9. the train step -----------------------------------------------------------------------------------------
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
    return float(loss), grads


def _close(gu, gf):
    """the bars of test_depth_grad_gpu.py::test_train_step_with_depth_loss on the parameter gradients"""
    assert gf.keys() == gu.keys()
    for k in gu:
        a, b = gu[k], gf[k]
        scale = max(a.abs().max().item(), 1e-30)
        d = (a - b).abs().flatten() / scale
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k


def test_train_step_with_mask_loss():
    """One fine-stage step with lambda_mask = 0.5 on (camera, gt, gt_depth or None, gt_mask) views, the masks (and
    depths) rendered from a perturbed model: the fused loss (gs4d_aux_loss_grad, one autograd.backward) against the
    unfused one (torch autograd), the optimizer held back so the parameter gradients are compared, for the mask
    alone and for mask + depth; then lambda_mask = 0 with 4-tuple views is the pair-view step bit for bit."""
    from gs4d_train import config
    from gs4d_train.render import render
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    W, H, P = 64, 48, 3000
    hyper, opt = config.dynerf()
    opt.iterations = 0
    pts, cols = make_point_cloud(P, seed=5)
    pairs = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")
    moved = (pts + np.random.default_rng(8).normal(0, 0.05, pts.shape)).astype(np.float32)
    other = _train_model(moved, cols, opt, hyper)
    quads, masked = [], []
    with torch.no_grad():
        for i, (cam, gt) in enumerate(pairs):
            pkg = render(cam, other, False, bg, alpha=True)
            assert set(pkg.keys()) == {"render", "viewspace_points", "radii", "depth", "alpha", "visibility_filter"}
            mask = pkg["alpha"].clone()
            assert mask.shape == (1, H, W) and 0.0 <= float(mask.min()) < float(mask.max()) <= 1.0
            quads.append((cam, gt, pkg["depth"].clone(), mask[0] if i == 1 else mask))  # (H, W) is accepted as well
            masked.append((cam, gt, None, mask))
        assert set(render(pairs[0][0], other, False, bg).keys()) == {"render", "viewspace_points", "radii", "depth",
                                                                     "visibility_filter"}
    opt.lambda_mask = 0.5
    l0, g0 = _step_grads(pts, cols, pairs, opt, hyper, fused_loss=True)
    # the mask alone
    lf, gf = _step_grads(pts, cols, masked, opt, hyper, fused_loss=True)
    lu, gu = _step_grads(pts, cols, masked, opt, hyper, fused_loss=False)
    print(f"[alpha-train] mask: fused {lf:.7g} unfused {lu:.7g} pairs {l0:.7g}", flush=True)
    assert abs(lf - lu) <= 1e-5 * abs(lu) and lf > l0
    assert not torch.equal(gf["_xyz"], g0["_xyz"])  # the mask term reached the Gaussians
    _close(gu, gf)
    # mask + depth
    opt.lambda_depth = 0.5
    lf2, gf2 = _step_grads(pts, cols, quads, opt, hyper, fused_loss=True)
    lu2, gu2 = _step_grads(pts, cols, quads, opt, hyper, fused_loss=False)
    print(f"[alpha-train] mask + depth: fused {lf2:.7g} unfused {lu2:.7g}", flush=True)
    assert abs(lf2 - lu2) <= 1e-5 * abs(lu2) and lf2 > lf
    _close(gu2, gf2)
    # lambda_mask = 0: 4-tuple views are pair views
    opt.lambda_depth = 0.0
    opt.lambda_mask = 0.0
    for fused, ref in ((True, (l0, g0)), (False, None)):
        lt, gt_ = _step_grads(pts, cols, masked, opt, hyper, fused_loss=fused)
        lp, gp = ref if ref is not None else _step_grads(pts, cols, pairs, opt, hyper, fused_loss=fused)
        assert lt == lp and gt_.keys() == gp.keys()
        for k in gp:
            assert torch.equal(gt_[k], gp[k]), k
