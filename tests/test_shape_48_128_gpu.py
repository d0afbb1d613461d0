"""The HyperNeRF / DyCheck shape (F, W) = (48, 128) (arguments/hypernerf/default.py, arguments/dycheck/default.py:
multires [1, 2, 4] x output_coordinate_dim 16, net_width 128) through the three kernels that carry the deformation
MLP's first layer -- gs4d_feature_relu_forward[_hb], gs4d_feature_relu_backward, gs4d_deform_infer -- and through the
Python layers above them (gs4d_train.infer, Deformation's fused heads, train_step), against float64 torch.

Bars.  First layer: an ordered f32 sum of K exact products errs by at most (K - 1) 2^-24 of its |terms| sum, 2.8e-6
at K = 48 and 7.6e-6 at K = 128, so the project's 1e-5 of the |terms| sum (test_feature_relu_backward_matches_fp64)
holds by derivation.  gs4d_deform_infer and the module: the carried bars of tests/test_infer_gpu.py, restated here
(_chain, _reference_bars, _activated_bars), with the fp32 torch formulation as a control.  Training: the bars of
test_train_step_fused_matches_torch_tail (1e-3 of a gradient tensor's maximum, 1e-4 at its 99.9th percentile) and of
test_train_step_bf16_mlp_tracks_fp32 (5 % relative L2)."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FIN, FOUT = 48, 128
POS, SCALES, ROT, OPACITY, SHS = range(5)
ROLE_N = (3, 3, 4, 1, 48)
HEAD_SETS = {"all five": [POS, SCALES, ROT, OPACITY, SHS], "no_do, no_dshs": [POS, SCALES, ROT], "rot only": [ROT],
             "shs only": [SHS]}
# empty, single, one short of and one past a 16-row block, ragged; then one point block past a full round of the
# grid's workgroups (1024 / k workgroups of 8 waves x 16 points): a second round of blocks per wave
POINTS = [0, 1, 15, 17, 777, 5003]
SECOND_ROUND = {"all five": 26_129, "no_do, no_dshs": 43_665}
EPS32 = 2.0 ** -24


# ---- the first layer: gs4d_feature_relu_forward[_hb] / gs4d_feature_relu_backward ----------------------------

# 0: zero gradients; 1; around one 16-row block; around one workgroup's four waves; ragged; 100_003: both kernels'
# grid-stride loops run more than once (the backward's grid caps at 512 workgroups = 32,768 rows, the forward's at 1024)
@pytest.mark.parametrize("P", [0, 1, 15, 16, 17, 63, 64, 65, 777, 100_003])
def test_feature_relu_48_128_matches_fp64(P):
    from gs4d_train import _C
    from gs4d_train.deformation import _FeatureReLU
    assert (FIN, FOUT) in _FeatureReLU.shapes
    torch.manual_seed(P + FIN)
    x = torch.randn(P, FIN, device="cuda")
    w = torch.randn(FOUT, FIN, device="cuda") * 0.2
    b = torch.randn(FOUT, device="cuda") * 0.1
    g = torch.randn(P, FOUT, device="cuda")
    # forward: h to 1e-5 of its row's |terms| sum, exact zeros where the ReLU clips; the bf16 copy; repeatable
    h = _C.feature_relu_forward(x, w, b)[0]
    h2, hb = _C.feature_relu_forward(x, w, b, with_hb=True)
    assert h.shape == (P, FOUT) and torch.equal(h2, h) and torch.equal(_C.feature_relu_forward(x, w, b)[0], h)
    assert hb.dtype == torch.bfloat16 and hb.shape == (P, FOUT) and torch.equal(hb, h.to(torch.bfloat16))
    if P:
        ref_h = x.double() @ w.double().t() + b.double()
        hscale = x.double().abs() @ w.double().abs().t() + b.double().abs()
        fh = float(((h.double() - ref_h.clamp_min(0)).abs() / hscale).max())
        print(f"\n[48x128] P = {P}: h {fh:.2e} of its |terms| sum (bar 1e-5)")
        assert fh <= 1e-5
        assert bool((h[ref_h < -1e-5 * hscale] == 0).all()) and 0.2 < float((h > 0).float().mean()) < 0.8
    # backward on the kernel's own h (its mask): dx per row, dW / db against their largest |terms| sum
    dx, dw, db = _C.feature_relu_backward(g, h, x, w)
    assert dx.shape == x.shape and dw.shape == w.shape and db.shape == (FOUT,)
    rd = (g * (h > 0)).double()
    rw, rb = rd.t() @ x.double(), rd.sum(0)
    if P:
        ref_dx, scale = rd @ w.double(), rd.abs() @ w.double().abs()
        fx = float(((dx.double() - ref_dx).abs() / scale.clamp_min(1e-300)).max())
        sw = (rd.abs().t() @ x.double().abs()).max().clamp_min(1e-30)
        sb = rd.abs().sum(0).max().clamp_min(1e-30)
        fw, fb = float((dw.double() - rw).abs().max() / sw), float((db.double() - rb).abs().max() / sb)
        print(f"[48x128] P = {P}: dx {fx:.2e} of its row's |terms| sum, dW {fw:.2e}, db {fb:.2e} of the largest (bar 1e-5)")
        assert fx <= 1e-5 and fw <= 1e-5 and fb <= 1e-5
    else:
        assert not bool(dw.any()) and not bool(db.any())
    # rows whose h <= 0 contribute exactly nothing: whatever their g holds (NaN), the results keep their bits
    gn = torch.where(h > 0, g, torch.full_like(g, float("nan")))
    for got, want in zip(_C.feature_relu_backward(gn, h, x, w), (dx, dw, db)):
        assert torch.equal(got, want)
    # two calls give the same bits
    for got, want in zip(_C.feature_relu_backward(g, h, x, w), (dx, dw, db)):
        assert torch.equal(got, want)
    # the autograd Function end to end: the raw bindings' bits
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    ha = _FeatureReLU.apply(xa, wa, ba)
    assert torch.equal(ha, h)
    ha.backward(g)
    assert torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw) and torch.equal(ba.grad, db)


# ---- gs4d_deform_infer: raw outputs against the fp64 chain (tests/test_infer_gpu.py's bars, restated) -------------

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
    """{role: (d, e_d)} of the heads in `dtype`; e_d, the bar carried through the three layers at 1e-5 of each
    layer's |terms| sum (ReLU is 1-Lipschitz), is formed only in float64"""
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


def _check_activated(raw, act, what):
    """each activated output against torch's activation of the kernel's own raw output, rtol = atol = 1e-6;
    means and SHs are not activated"""
    m3, sc, rot, op, sh = raw
    assert torch.equal(act[0], m3) and torch.equal(act[4], sh), what
    for got, want in ((act[1], torch.exp(sc)), (act[2], F.normalize(rot)), (act[3], torch.sigmoid(op))):
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("heads", list(HEAD_SETS))
def test_deform_infer_48_128_raw_matches_fp64(heads):
    roles = HEAD_SETS[heads]
    worst, worst_ctl = 0.0, 0.0
    for P in POINTS + ([SECOND_ROUND[heads]] if heads in SECOND_ROUND else []):
        net, base = _inputs(P, FIN, FOUT, roles, seed=P + 7 * FOUT + FIN + len(roles))
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
        act = _run(net, base, roles, True)
        _check_activated(outs, act, f"{heads}, P = {P}")
        assert all(torch.equal(x, y) for x, y in zip(_run(net, base, roles, True), act))
    print(f"\n[48x128] deform_infer raw, {heads}: kernel {worst:.3f} of the bar, fp32 torch control {worst_ctl:.3f}")
    assert worst_ctl <= 1.0, "the fp32 torch formulation itself exceeds the bar: the bar is wrong, not the kernel"
    assert worst <= 1.0


def test_deform_infer_48_128_zero_quaternion_stays_zero():
    P = 777
    # without a rot head: a zero base row passes through, activated
    roles = [POS, SCALES]
    net, base = _inputs(P, FIN, FOUT, roles, seed=4)
    base["r"][5] = 0.0
    raw, act = _run(net, base, roles, False), _run(net, base, roles, True)
    assert torch.equal(raw[2], base["r"]) and bool((act[2][5] == 0).all()) and bool(torch.isfinite(act[2]).all())
    _check_activated(raw, act, "pass-through")
    # the rot head with a zero second layer over a zero base row: r + dr = 0 inside the head's epilogue
    roles = [ROT]
    net, base = _inputs(P, FIN, FOUT, roles, seed=5)
    net["w2"][0].zero_()
    net["b2"][0].zero_()
    base["r"][9] = 0.0
    raw, act = _run(net, base, roles, False), _run(net, base, roles, True)
    assert bool((raw[2][9] == 0).all()) and bool((act[2][9] == 0).all()) and bool(torch.isfinite(act[2]).all())
    _check_activated(raw, act, "zero quaternion in the rot head")


# ---- gs4d_train.infer on a model with the HyperNeRF preset -------------------------------------------------------

def _hyper(**over):
    from gs4d_train import config
    return config.model_hidden_params(**{**config.HYPERNERF_HIDDEN, **over})


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


@functools.lru_cache(maxsize=None)
def _shared_model(all_heads):
    return _model(_hyper(no_do=False, no_dshs=False) if all_heads else _hyper(), seed=3 if all_heads else 2)


def _reference_bars(g, t):
    """(fp64 raw outputs, their bars) of the unfused torch graph of g in float64: the field by F.grid_sample
    (grid.fused = False), then _chain with e_feat = 1e-5 max |feat| at its head, the field's bar in
    test_hexplane_fused_matches_reference_module."""
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


@pytest.mark.parametrize("all_heads", [False, True], ids=["preset heads", "all five heads"])
def test_infer_serves_the_hypernerf_preset(all_heads):
    """prepare() takes the fused path; state_at_time within the fp64 unfused graph's bars; a row permutation of the
    model permutes the outputs bitwise; render_view renders.  all five heads: the LDS-largest head set (shs)."""
    from gs4d_train import infer
    from gs4d_train.synthetic import look_at_camera
    g = _shared_model(all_heads)
    net = g._deformation.deformation_net
    assert net.grid.feat_dim == FIN and net.W == FOUT and len(net.grid.grids) == 3
    state = infer.prepare(g)
    assert state.fused is True
    assert len(state.roles) == (5 if all_heads else 3)
    for t in (0.0, 0.37, 1.0):
        fr, fa = _state_fracs(infer.state_at_time(state, t, activate=False), infer.state_at_time(state, t), g, t)
        print(f"\n[48x128] state t = {t}, {len(state.roles)} heads: raw {fr:.3f} of the bar, activated {fa:.3f}")
        assert fr <= 1.0 and fa <= 1.0
    a, b = infer.state_at_time(state, 0.37), infer.state_at_time(state, 0.37)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.randperm(g._xyz.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    g2 = copy.copy(g)
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
        setattr(g2, n, torch.nn.Parameter(getattr(g, n).detach()[perm].contiguous()))
    for x, y in zip(a, infer.state_at_time(infer.prepare(g2), 0.37)):
        assert torch.equal(x[perm], y)
    cam = look_at_camera(64, 48, (4.0 * math.sin(0.3), 0.4, -4.0 * math.cos(0.3)), time=0.5)
    pkg = infer.render_view(cam, state, torch.ones(3, device="cuda"))
    assert tuple(pkg["render"].shape) == (3, 48, 64) and tuple(pkg["depth"].shape)[-2:] == (48, 64)
    assert tuple(pkg["radii"].shape) == (2000,) and int(pkg["visibility_filter"].sum()) > 100
    assert bool(torch.isfinite(pkg["render"]).all()) and bool(torch.isfinite(pkg["depth"]).all())


# ---- training: Deformation's fused heads and train_step at the preset ----------------------------------------

def _count_calls(monkeypatch, name):
    """a counter wrapped around gs4d_train._C.<name>: [calls, calls with with_hb=True]"""
    from gs4d_train import _C
    real = getattr(_C, name)
    calls = [0, 0]

    def counted(*a, **k):
        calls[0] += 1
        calls[1] += bool(k.get("with_hb", False))
        return real(*a, **k)
    monkeypatch.setattr(_C, name, counted)
    return calls


def _deformation(seed, mlp_dtype="fp32"):
    """A Deformation with the preset on the GPU, fused field and heads, the planes and Linears re-drawn as _model's"""
    from gs4d_train.deformation import Deformation
    hyper = _hyper(mlp_dtype=mlp_dtype)
    torch.manual_seed(seed)
    net = Deformation(W=hyper.net_width, D=hyper.defor_depth, args=hyper).cuda()
    net.grid.fused = net.fused_heads = True
    with torch.no_grad():
        for level in net.grid.grids:
            for p in level:
                p.copy_(torch.rand_like(p) * 0.4 + 0.1)
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn_like(m.weight) / m.in_features ** 0.5)
                m.bias.copy_(0.1 * torch.randn_like(m.bias))
    return net


def _deformation_inputs(P, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    xyz = torch.rand(P, 3, generator=g) * 2.4 - 1.2
    ins = [xyz, rn(P, 3), rn(P, 4), rn(P, 1), rn(P, 16, 3)]
    ups = [rn(P, 3), rn(P, 3), rn(P, 4)]
    to = lambda t: t.to(device="cuda", dtype=dtype)
    time = torch.full((P, 1), float(np.float32(0.37)), dtype=dtype, device="cuda")
    return [to(t) for t in ins], [to(t) for t in ups], time


def _deformation_grads(net, P, seed, dtype=torch.float32):
    """(outputs, {name: gradient}) of sum(out * upstream) over the three deformed outputs: every parameter that
    receives a gradient, and the points"""
    ins, ups, time = _deformation_inputs(P, seed, dtype)
    ins[0].requires_grad_(True)
    net.zero_grad(set_to_none=True)
    outs = net(*ins, time)
    sum((o * u).sum() for o, u in zip(outs[:3], ups)).backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    grads["xyz"] = ins[0].grad.detach().clone()
    return [o.detach() for o in outs], grads


def _tie_free(net, P, seed, margin=1e-7):
    """No ReLU input of the fp64 graph within `margin` of zero.  A pre-activation that close to zero may take the
    other side of the ReLU in fp32, which flips one whole row's term in a weight gradient: the input's conditioning
    and no kernel's error.  The margin is the first layer's rounding bound at these inputs, 2.8e-6 of a |terms| sum
    of about 0.1 (features of 1e-3, weights and biases of 0.1) less a little; about one draw in three passes."""
    net64 = copy.deepcopy(net).double()
    net64.grid.fused = net64.fused_heads = False
    ins, _, time = _deformation_inputs(P, seed, torch.float64)
    with torch.no_grad():
        z = net64.feature_out(net64.grid(ins[0], time))
        zs = [z] + [hd[1](torch.relu(z)) for hd in (net64.pos_deform, net64.scales_deform, net64.rotations_deform)]
    return min(float(t.abs().min()) for t in zs) >= margin


def test_deformation_fused_heads_run_the_first_layer_kernel(monkeypatch):
    """Deformation with the preset, fused_heads = True, P = 3000: the fused first layer runs (a counter around
    _C.feature_relu_forward); every parameter's and the points' gradient against the fp64 unfused graph at the
    train step's bars; two runs from identically seeded fresh models are bitwise equal."""
    P = 3000
    seed = next(s for s in range(11, 75) if _tie_free(_deformation(s), P, s))
    fwd = _count_calls(monkeypatch, "feature_relu_forward")
    bwd = _count_calls(monkeypatch, "feature_relu_backward")
    net = _deformation(seed)
    assert net.grid.feat_dim == FIN and net.W == FOUT
    outs, grads = _deformation_grads(net, P, seed)
    assert fwd[0] == 1 and bwd[0] == 1, "the fused first layer did not run"
    net64 = copy.deepcopy(net).double()
    net64.grid.fused = net64.fused_heads = False
    outs64, grads64 = _deformation_grads(net64, P, seed, torch.float64)
    assert fwd[0] == 1 and bwd[0] == 1  # the reference is the torch graph
    assert grads.keys() == grads64.keys() and "feature_out.0.weight" in grads and "grid.grids.2.5" in grads
    for got, want in zip(outs[:3], outs64[:3]):
        assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    worst = 0.0
    for k in grads:
        a, b = grads64[k], grads[k].double()
        d = (a - b).abs().flatten() / max(a.abs().max().item(), 1e-30)
        worst = max(worst, d.max().item())
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k
    print(f"\n[48x128] Deformation P = {P}, seed {seed}: largest gradient error {worst:.2e} of its tensor's max (bar 1e-3)")
    outs2, grads2 = _deformation_grads(_deformation(seed), P, seed)
    assert all(torch.equal(x, y) for x, y in zip(outs, outs2))
    assert all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_deformation_bf16_heads_read_the_hb_copy(monkeypatch):
    """mlp_dtype = "bf16": the first layer's kernel also writes the bf16 copy of h the heads block reads (counter),
    and the deltas stay within the bf16 step's bar, 5 % relative L2 of the fp32 path's."""
    P, seed = 3000, 11
    fwd = _count_calls(monkeypatch, "feature_relu_forward")
    outs, _ = _deformation_grads(_deformation(seed), P, seed)
    assert fwd == [1, 0]
    outs_b, grads_b = _deformation_grads(_deformation(seed, "bf16"), P, seed)
    assert fwd == [2, 1], "the bf16 path did not take the first layer's hb copy"
    ins, _, _ = _deformation_inputs(P, seed)
    for name, x, y, base in zip(("pos", "scales", "rot"), outs_b[:3], outs[:3], ins[:3]):
        assert x.dtype == torch.float32
        rel = float((x - y).norm() / (y - base).norm())
        print(f"\n[48x128] bf16 {name} delta: {rel:.2e} relative L2 of the fp32 delta (bar 5e-2)")
        assert rel <= 5e-2, (name, rel)
    assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in grads_b.values())


def test_train_step_at_the_preset_fused_matches_torch_tail(monkeypatch):
    """One fine-stage step at the HyperNeRF preset (P = 20,000, 320x240, two views), fused against the reference's
    torch formulation, with test_train_step_fused_matches_torch_tail's tolerances; the fused step repeated from the
    same state gives the same bits."""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    hyper, opt = config.hypernerf()
    opt.iterations = 0  # the optimizer is held back: the gradients themselves are compared
    pts, cols = make_point_cloud(20000, seed=5)
    views = make_training_views(2, 320, 240, seed=6)
    bg = torch.ones(3, device="cuda")
    fwd = _count_calls(monkeypatch, "feature_relu_forward")
    runs = []
    for fused in (False, True, True):
        torch.manual_seed(7)
        g = GaussianModel(3, hyper, fused=fused)
        g.create_from_pcd(pts, cols, 1.0)
        g._deformation.deformation_net.grid.fused = fused
        g._deformation.deformation_net.fused_heads = fused
        g.training_setup(opt)
        g.active_sh_degree = 3
        before = fwd[0]
        loss = float(train_step(g, views, opt, hyper, 3001, bg))
        assert (fwd[0] > before) == fused
        grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            grads[name] = getattr(g, name).grad.detach().clone()
        runs.append((g, loss, grads))
    (ga, la, gra), (gb, lb, grb), (gc, lc, grc) = runs
    assert tuple(gb._deformation.deformation_net.feature_out[0].weight.shape) == (FOUT, FIN)
    assert abs(lb - la) <= 1e-5 * abs(la)
    assert gra.keys() == grb.keys() == grc.keys()
    for k in gra:
        a, b = gra[k], grb[k]
        d = (a - b).abs().flatten() / max(a.abs().max().item(), 1e-30)
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k
    acc_scale = max(ga.xyz_gradient_accum.abs().max().item(), 1e-30)
    d = (gb.xyz_gradient_accum - ga.xyz_gradient_accum).abs().flatten() / acc_scale
    assert d.max().item() < 1e-3, d.max().item()
    assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4
    assert torch.equal(gb.denom, ga.denom) and torch.equal(gb.max_radii2D, ga.max_radii2D)
    # repeated: bitwise
    assert lc == lb and all(torch.equal(grb[k], grc[k]) for k in grb)
    assert torch.equal(gc.xyz_gradient_accum, gb.xyz_gradient_accum)
