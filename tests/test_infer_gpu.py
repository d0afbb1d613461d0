"""The inference path on the GPU: gs4d_deform_infer (csrc/deform_infer.hip) against the torch formulation in
float64 on the same fp32 inputs, and gs4d_train.infer (prepare / state_at_time / render_view / render_set /
evaluate) against the reference module's graph and the existing render().

Bars.  The kernel writes no intermediate, so the project's per-layer bar -- 1e-5 of the |terms| sum of a
layer's dot products (test_heads_block_forward_matches_fp64 and its neighbours) -- is carried through the chain
with every term taken from the fp64 values (ReLU is 1-Lipschitz):
    e_h = 1e-5 (|feat| |Wf|^T + |bf|)  [+ e_feat |Wf|^T when the features themselves carry an error]
    e_a = 1e-5 (|h| |W1|^T + |b1|) + e_h |W1|^T
    e_d = 1e-5 (|a| |W2|^T + |b2|) + e_a |W2|^T
and a raw output base + d must lie within e_d plus one fp32 rounding of the add, 2^-24 (|base + d| + e_d), at
every element.  The fp32 torch formulation runs on the same inputs as a control: were IT to exceed a bar, the bar
would be wrong, and the test says so.  Each test prints the largest fraction of its bar it used ([infer-bars])."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

POS, SCALES, ROT, OPACITY, SHS = range(5)
ROLE_N = (3, 3, 4, 1, 48)
SHAPES = [(32, 128), (64, 64), (32, 64)]
HEAD_SETS = {"all five": [POS, SCALES, ROT, OPACITY, SHS], "no_do, no_dshs": [POS, SCALES, ROT], "rot only": [ROT],
             "shs only": [SHS]}
POINTS = [0, 1, 15, 17, 777, 5003]  # empty, single, one short of and one past a 16-row block, ragged
EPS32 = 2.0 ** -24


def _inputs(P, Fdim, W, roles, seed):
    """weights randn / sqrt(fan_in), biases 0.1 randn, feat products of U(0.1, 0.5) values like the field's"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    feat = (torch.rand(P, Fdim, 6, device="cuda", generator=g) * 0.4 + 0.1).prod(-1)
    k = len(roles)
    net = dict(feat=feat, wf=rn(W, Fdim) / Fdim ** 0.5, bf=0.1 * rn(W), w1=rn(k * W, W) / W ** 0.5, b1=0.1 * rn(k * W),
               w2=[rn(ROLE_N[r], W) / W ** 0.5 for r in roles], b2=[0.1 * rn(ROLE_N[r]) for r in roles])
    base = dict(xyz=rn(P, 3), s=rn(P, 3), r=rn(P, 4), o=rn(P, 1), f_dc=rn(P, 1, 3), f_rest=rn(P, 15, 3))
    return net, base


def _run(net, base, roles, activate):
    from gs4d_train import _C
    return _C.deform_infer(net["feat"], net["wf"], net["bf"], net["w1"], net["b1"], net["w2"], net["b2"], list(roles),
                           base["xyz"], base["s"], base["r"], base["o"], base["f_dc"], base["f_rest"], activate)


def _bases(base):
    return [base["xyz"], base["s"], base["r"], base["o"], torch.cat((base["f_dc"], base["f_rest"]), 1)]


def _chain(net, roles, dtype, e_feat=0.0):
    """{role: (d, e_d)} of the heads in `dtype`; e_d (the carried bar) is formed only in float64"""
    c = lambda t: t.to(dtype)
    feat, wf, bf = c(net["feat"]), c(net["wf"]), c(net["bf"])
    W = wf.shape[0]
    h = torch.relu(feat @ wf.t() + bf)
    bars = dtype == torch.float64
    if bars:
        e_h = 1e-5 * (feat.abs() @ wf.abs().t() + bf.abs()) + e_feat * wf.abs().sum(1)
    out = {}
    for i, r in enumerate(roles):
        w1, b1 = c(net["w1"][i * W:(i + 1) * W]), c(net["b1"][i * W:(i + 1) * W])
        w2, b2 = c(net["w2"][i]), c(net["b2"][i])
        a = torch.relu(h @ w1.t() + b1)
        d = a @ w2.t() + b2
        e_d = None
        if bars:
            e_a = 1e-5 * (h.abs() @ w1.abs().t() + b1.abs()) + e_h @ w1.abs().t()
            e_d = 1e-5 * (a.abs() @ w2.abs().t() + b2.abs()) + e_a @ w2.abs().t()
        out[r] = (d, e_d)
    return out


def _frac(got, want, bar):
    """largest |got - want| / bar over the elements (inf for a non-finite result)"""
    if got.numel() == 0:
        return 0.0
    err = (got.double() - want).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err / bar).max())


@pytest.mark.parametrize("heads", list(HEAD_SETS))
@pytest.mark.parametrize("Fdim,W", SHAPES)
def test_deform_infer_raw_matches_fp64(Fdim, W, heads):
    roles = HEAD_SETS[heads]
    worst, worst_ctl = 0.0, 0.0
    for P in POINTS:
        net, base = _inputs(P, Fdim, W, roles, seed=P + 7 * W + Fdim + len(roles))
        outs = _run(net, base, roles, False)
        assert [tuple(o.shape) for o in outs] == [(P, 3), (P, 3), (P, 4), (P, 1), (P, 16, 3)]
        if P == 0:
            continue
        ref, ctl = _chain(net, roles, torch.float64), _chain(net, roles, torch.float32)
        for role, (got, b) in enumerate(zip(outs, _bases(base))):
            if role not in roles:
                assert torch.equal(got, b), f"role {role} has no head: its base must pass through bitwise (P={P})"
                continue
            d, e_d = ref[role]
            want = b.double().reshape(P, -1) + d
            bar = e_d + EPS32 * (want.abs() + e_d)
            worst = max(worst, _frac(got.reshape(P, -1), want, bar))
            worst_ctl = max(worst_ctl, _frac(b.reshape(P, -1) + ctl[role][0], want, bar))
    print(f"\n[infer-bars] raw (F, W) = ({Fdim}, {W}), {heads}: kernel {worst:.3f} of the bar, "
          f"fp32 torch control {worst_ctl:.3f}")
    assert worst_ctl <= 1.0, "the fp32 torch formulation itself exceeds the bar: the bar is wrong, not the kernel"
    assert worst <= 1.0


def _check_activated(raw, act, what):
    """each activated output against torch's activation of the kernel's own raw output, rtol = atol = 1e-6
    (deform_tail's bar in test_deform_tail_matches_torch); means and SHs are not activated"""
    m3, sc, rot, op, sh = raw
    assert torch.equal(act[0], m3) and torch.equal(act[4], sh), what
    for got, want in ((act[1], torch.exp(sc)), (act[2], F.normalize(rot)), (act[3], torch.sigmoid(op))):
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6, msg=lambda m: f"{what}: {m}")


def test_deform_infer_activations_match_torch():
    P = 777
    # (32, 128), all five heads; rows whose s + ds is +-80 (finite either way) and +-120 (inf and exactly 0)
    roles = HEAD_SETS["all five"]
    net, base = _inputs(P, 32, 128, roles, seed=3)
    ds = _run(net, base, roles, False)[1] - base["s"]
    for row, v in enumerate((80.0, -80.0, 120.0, -120.0)):
        base["s"][row] = v - ds[row]
    raw, act = _run(net, base, roles, False), _run(net, base, roles, True)
    assert float((raw[1][:4] - torch.tensor([[80.0], [-80.0], [120.0], [-120.0]], device="cuda")).abs().max()) < 1e-3
    assert bool(torch.isinf(act[1][2]).all()) and bool((act[1][3] == 0).all())
    assert bool(torch.isfinite(act[1][:2]).all()) and bool((act[1][:2] > 0).all())
    _check_activated(raw, act, "all five heads")
    # (64, 64), rot / opacity / shs pass through activated; a zero quaternion among the bases
    roles = [POS, SCALES]
    net, base = _inputs(P, 64, 64, roles, seed=4)
    base["r"][5] = 0.0
    raw, act = _run(net, base, roles, False), _run(net, base, roles, True)
    assert torch.equal(raw[2], base["r"]) and bool((act[2][5] == 0).all()) and bool(torch.isfinite(act[2]).all())
    _check_activated(raw, act, "pass-through")
    # (32, 64), the rot head with a zero second layer over a zero base row: r + dr = 0 inside the head's epilogue
    roles = [ROT]
    net, base = _inputs(P, 32, 64, roles, seed=5)
    net["w2"][0].zero_()
    net["b2"][0].zero_()
    base["r"][9] = 0.0
    raw, act = _run(net, base, roles, False), _run(net, base, roles, True)
    assert bool((raw[2][9] == 0).all()) and bool((act[2][9] == 0).all()) and bool(torch.isfinite(act[2]).all())
    _check_activated(raw, act, "zero quaternion in the rot head")


# ---- the Python module --------------------------------------------------------------------------------------

def _model(hyper, P=2000, seed=0):
    """A GaussianModel of P random points in the field's bounds, the planes moved off their initial values (the time
    planes start at exactly 1) and every Linear of the MLP re-drawn (randn / sqrt(fan_in), bias 0.1 randn) so that
    the deltas are O(0.1)."""
    from gs4d_train.gaussians import GaussianModel
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=True)
    g._deformation = g._deformation.cuda()
    par = lambda t: torch.nn.Parameter(t.cuda())
    g._xyz = par(torch.rand(P, 3) * 2.4 - 1.2)
    g._scaling = par(torch.randn(P, 3) * 0.3 - 3.0)
    g._rotation = par(torch.randn(P, 4))
    g._opacity = par(torch.randn(P, 1))
    g._features_dc = par(torch.randn(P, 1, 3) * 0.5)
    g._features_rest = par(torch.randn(P, 15, 3) * 0.1)
    g.active_sh_degree = 3
    net = g._deformation.deformation_net
    net.grid.fused = True
    net.fused_heads = True
    with torch.no_grad():
        for level in net.grid.grids:
            for p in level:
                p.copy_(torch.rand_like(p) * 0.4 + 0.1)
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn_like(m.weight) / m.in_features ** 0.5)
                m.bias.copy_(0.1 * torch.randn_like(m.bias))
    return g


def _hyper(name, **over):
    from gs4d_train import config
    base = config.DNERF_HIDDEN if name == "dnerf" else config.DYNERF_HIDDEN
    return config.model_hidden_params(**{**base, **over})


@functools.lru_cache(maxsize=None)
def _shared_model(name):
    return _model(_hyper(name), seed=1 if name == "dnerf" else 2)


def _reference_bars(g, t):
    """(fp64 raw outputs, their bars) of the unfused torch graph of g in float64: the field by F.grid_sample
    (grid.fused = False), then the chain of the module docstring with e_feat = 1e-5 max |feat| at its head, the
    field's bar in test_hexplane_fused_matches_reference_module."""
    net64 = copy.deepcopy(g._deformation.deformation_net).double()
    net64.grid.fused = False
    net64.fused_heads = False
    a = net64.args
    names = ("pos_deform", "scales_deform", "rotations_deform", "opacity_deform", "shs_deform")
    roles = [r for r, flag in enumerate((a.no_dx, a.no_ds, a.no_dr, a.no_do, a.no_dshs)) if not flag]
    with torch.no_grad():
        P = g._xyz.shape[0]
        time = torch.full((P, 1), float(np.float32(t)), dtype=torch.float64, device="cuda")
        feat = net64.grid(g._xyz.detach().double(), time)
        W = net64.W
        lin = net64.feature_out[0]
        net = dict(feat=feat, wf=lin.weight, bf=lin.bias,
                   w1=torch.cat([getattr(net64, names[r])[1].weight for r in roles]),
                   b1=torch.cat([getattr(net64, names[r])[1].bias for r in roles]),
                   w2=[getattr(net64, names[r])[3].weight for r in roles],
                   b2=[getattr(net64, names[r])[3].bias for r in roles])
        chain = _chain(net, roles, torch.float64, e_feat=1e-5 * float(feat.abs().max()))
        bases = [g._xyz, g._scaling, g._rotation, g._opacity, g.get_features]
        raw, bars = [], []
        for role, b in enumerate(bases):
            b = b.detach().double().reshape(P, -1)
            if role in chain:
                d, e_d = chain[role]
                raw.append(b + d)
                bars.append(e_d + EPS32 * ((b + d).abs() + e_d))
            else:
                raw.append(b)
                bars.append(torch.zeros_like(b))
        # the chain restates the module: its own forward gives the same fp64 values
        ref = net64(*[x.detach().double() for x in bases], time)
        for x, y in zip(raw, ref):
            assert float((x - y.reshape(P, -1)).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
    return raw, bars


def _activated_bars(raw, bars):
    """The activations' effect on a raw bar e, each function's own Lipschitz bound, plus 4 fp32 roundings of
    the activated value for the activation's own arithmetic: exp(x + e) - exp(x) <= exp(x) expm1(e); a unit
    quaternion moves by at most 2 |e|_2 / |q| when q moves by e; sigmoid' <= 1 / 4."""
    m3, sc, rot, op, sh = raw
    e3, es, er, eo, esh = bars
    ulp = 4 * EPS32
    act = [m3, torch.exp(sc), F.normalize(rot), torch.sigmoid(op), sh]
    nrm = rot.norm(dim=1, keepdim=True)
    abars = [e3, torch.exp(sc) * torch.expm1(es) + ulp * torch.exp(sc),
             (2 * er.norm(dim=1, keepdim=True) / nrm).expand_as(rot) + ulp, eo / 4 + ulp, esh]
    return act, abars


def _state_fracs(got_raw, got_act, g, t):
    raw, bars = _reference_bars(g, t)
    act, abars = _activated_bars(raw, bars)
    P = raw[0].shape[0]
    fr, fa = 0.0, 0.0
    for x, y, b in zip(got_raw, raw, bars):
        if float(b.max()) == 0.0:  # a role without a head: bitwise its base
            assert torch.equal(x.reshape(P, -1).double(), y)
        else:
            fr = max(fr, _frac(x.reshape(P, -1), y, b))
    for x, y, b in zip(got_act, act, abars):
        fa = max(fa, _frac(x.reshape(P, -1), y, b.clamp_min(1e-300)))
    return fr, fa


@pytest.mark.parametrize("name", ["dnerf", "dynerf"])
def test_state_at_time_matches_the_reference_graph_in_fp64(name):
    from gs4d_train import infer
    g = _shared_model(name)
    state = infer.prepare(g)
    assert state.fused is True
    for t in (0.0, 0.37, 1.0):
        fr, fa = _state_fracs(infer.state_at_time(state, t, activate=False), infer.state_at_time(state, t), g, t)
        print(f"\n[infer-bars] state {name} t = {t}: raw {fr:.3f} of the bar, activated {fa:.3f}")
        assert fr <= 1.0 and fa <= 1.0
    # get_state_at_time: the reference's tuple, the undeformed opacity parameter in it
    cam = type("Cam", (), {"time": 0.37})()
    got = infer.get_state_at_time(state, cam)
    raw = infer.state_at_time(state, 0.37, activate=False)
    assert all(torch.equal(a, b) for a, b in zip(got, (raw[0], raw[1], raw[2], g._opacity.detach(), raw[4])))


def test_state_is_deterministic_and_the_point_order_is_only_locality():
    from gs4d_train import infer
    g = _shared_model("dynerf")
    state = infer.prepare(g)
    a, b = infer.state_at_time(state, 0.37), infer.state_at_time(state, 0.37)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.randperm(g._xyz.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    g2 = copy.copy(g)
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
        setattr(g2, n, torch.nn.Parameter(getattr(g, n).detach()[perm].contiguous()))
    state2 = infer.prepare(g2)
    assert not torch.equal(state2.order, state.order)
    for x, y in zip(a, infer.state_at_time(state2, 0.37)):
        assert torch.equal(x[perm], y)


def test_state_is_a_capture():
    from gs4d_train import infer
    g = _model(_hyper("dnerf"), P=500, seed=3)
    state = infer.prepare(g)
    before = infer.state_at_time(state, 0.6)
    net = g._deformation.deformation_net
    with torch.no_grad():
        net.grid.grids[1][2].mul_(1.5)
        net.scales_deform[1].weight.add_(0.05)
    after = infer.state_at_time(state, 0.6)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    fresh = infer.prepare(g)
    got = infer.state_at_time(fresh, 0.6)
    assert not torch.equal(got[1], before[1])
    fr, fa = _state_fracs(infer.state_at_time(fresh, 0.6, activate=False), got, g, 0.6)
    print(f"\n[infer-bars] state after an in-place edit, prepared again: raw {fr:.3f} of the bar, activated {fa:.3f}")
    assert fr <= 1.0 and fa <= 1.0


@pytest.mark.parametrize("over", [dict(net_width=256), dict(defor_depth=2)])
def test_unsupported_shapes_take_the_torch_formulation(over):
    from gs4d_train import infer
    g = _model(_hyper("dnerf", **over), P=300, seed=4)
    state = infer.prepare(g)
    assert state.fused is False
    with torch.no_grad():
        time = torch.full((300, 1), float(np.float32(0.37)), device="cuda")
        m3, sc, rot, op, sh = g._deformation(g._xyz, g._scaling, g._rotation, g._opacity, g.get_features, time)
        want = (m3, torch.exp(sc), F.normalize(rot), torch.sigmoid(op), sh)
        raw = (m3, sc, rot, op, sh)
    assert all(torch.equal(x, y) for x, y in zip(infer.state_at_time(state, 0.37), want))
    assert all(torch.equal(x, y) for x, y in zip(infer.state_at_time(state, 0.37, activate=False), raw))


def test_coarse_stage_is_the_tail_alone():
    from gs4d_train import infer
    from gs4d_train.kernels import deform_tail
    g = _shared_model("dnerf")
    state = infer.prepare(g, "coarse")
    with torch.no_grad():
        want = deform_tail(g._xyz, g._scaling, g._rotation, g._opacity, g._features_dc, g._features_rest)
    assert all(torch.equal(x, y) for x, y in zip(infer.state_at_time(state, 0.37), want))
    raw = infer.state_at_time(state, 0.37, activate=False)
    assert torch.equal(raw[1], g._scaling.detach()) and torch.equal(raw[4], g.get_features.detach())


def _cameras(n, W=64, H=48):
    from gs4d_train.synthetic import look_at_camera
    return [look_at_camera(W, H, (4.0 * math.sin(0.3 * i), 0.4, -4.0 * math.cos(0.3 * i)), time=i / max(1, n - 1))
            for i in range(n)]


def test_render_view_is_the_rasterizer_on_the_state():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import infer
    from gs4d_train.render import render
    g = _shared_model("dnerf")
    cam = _cameras(3)[1]
    bg = torch.ones(3, device="cuda")
    state = infer.prepare(g)
    pkg = infer.render_view(cam, state, bg)
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    m3, sc, rot, op, sh = infer.state_at_time(state, cam.time)
    view_m, proj_m, cam_c = cam.on_device(torch.device("cuda:0"))
    settings = dgr.GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg,
        scale_modifier=1.0, viewmatrix=view_m, projmatrix=proj_m, sh_degree=3, campos=cam_c, prefiltered=False,
        debug=False)
    with torch.no_grad():
        image, radii, depth = dgr.GaussianRasterizer(raster_settings=settings)(
            means3D=m3, means2D=torch.zeros_like(m3), shs=sh, colors_precomp=None, opacities=op, scales=sc,
            rotations=rot, cov3D_precomp=None)
    assert torch.equal(pkg["render"], image) and torch.equal(pkg["radii"], radii) and torch.equal(pkg["depth"], depth)
    assert torch.equal(pkg["visibility_filter"], radii > 0) and int(pkg["visibility_filter"].sum()) > 100
    assert tuple(pkg["viewspace_points"].shape) == (2000, 3) and not bool(pkg["viewspace_points"].any())
    # against render(): d0 = what its two existing paths (fused / unfused, both under no_grad) differ by
    net = g._deformation.deformation_net
    try:
        with torch.no_grad():
            fused_img = render(cam, g, False, bg)["render"]
            g.fused = net.grid.fused = net.fused_heads = False
            unfused_img = render(cam, g, False, bg)["render"]
    finally:
        g.fused = net.grid.fused = net.fused_heads = True
    d0 = float((fused_img - unfused_img).abs().mean())
    d1 = float((pkg["render"] - unfused_img).abs().mean())
    print(f"\n[infer-bars] render_view 64x48: mean |render_view - unfused render()| = {d1:.3e}, "
          f"d0 = mean |fused render() - unfused render()| = {d0:.3e}")
    assert d1 <= 2 * d0 + 1e-6


def _ssim_map(img1, img2):
    """losses.ssim (utils/loss_utils.py:36-66) up to its map"""
    from gs4d_train.losses import create_window
    window = create_window(11, 3).to(device=img1.device, dtype=img1.dtype)
    conv = lambda x: F.conv2d(x, window, padding=5, groups=3)
    mu1, mu2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - mu1.pow(2), conv(img2 * img2) - mu2.pow(2), conv(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1.pow(2) + mu2.pow(2) + C1) * (s1 + s2 + C2))


def test_render_set_and_evaluate():
    from gs4d_train import infer, losses
    g = _shared_model("dnerf")
    cams = _cameras(6)
    bg = torch.ones(3, device="cuda")
    state = infer.prepare(g)
    images, fps = infer.render_set(state, cams, bg)
    assert len(images) == 6 and all(tuple(im.shape) == (3, 48, 64) for im in images)
    assert math.isfinite(fps) and fps > 0
    for cam, im in zip(cams, images):
        assert torch.equal(im, infer.render_view(cam, state, bg)["render"])
    none, fps2 = infer.render_set(state, cams, bg, keep_images=False)
    assert none == [] and math.isfinite(fps2) and fps2 > 0
    gen = torch.Generator(device="cuda").manual_seed(9)
    views = [(c, (im + 0.1 * torch.randn(im.shape, device="cuda", generator=gen)).clamp(0, 1)) for c, im in zip(cams, images)]
    got = infer.evaluate(state, views, bg)
    assert set(got) == {"psnr", "ssim"}
    psnrs, ssims, em = [], [], 0.0
    for (c, gt), im in zip(views, images):
        x, y = im.clamp(0, 1).unsqueeze(0), gt.unsqueeze(0)
        psnrs.append(float(losses.psnr(x, y).mean()))
        m64 = _ssim_map(x.double(), y.double())
        assert abs(float(m64.mean()) - float(losses.ssim(x.double(), y.double()))) <= 1e-14
        em = max(em, float((_ssim_map(x, y).double() - m64).abs().max()))
        ssims.append(float(m64.mean()))
    assert abs(got["psnr"] - float(np.mean(psnrs))) <= 1e-4
    # the fused SSIM value's documented bar (test_ssim_gpu.py): within 4 em of the fp64 value, em = the fp32
    # formulation's largest map error
    err = abs(got["ssim"] - float(np.mean(ssims)))
    print(f"\n[infer-bars] evaluate: psnr {got['psnr']:.3f} dB, ssim {got['ssim']:.6f}, ssim error {err:.2e} of bar {4 * em:.2e}")
    assert err <= 4 * em + EPS32
