"""GPU tests of the N-channel feature rendering (gs4d_features_forward / _backward and everything above them).

Two references (tests/feature_refs.py).  A, the composition: ceil(C / 3) calls of the rasterizer itself with three
channels at a time as colors_precomp over a zero background.  The fused forward must give its bits (same w, same fma,
same order; the forward's final write C + T * 0 keeps C), on every scene, termination, the cap and the 1/255 rule
included; the fused backward reads the same forward state, so no decision can flip and every element of every gradient
is held to the bar GRAD_RTOL |ref| + GRAD_FLOOR max |ref| (oracle/parity.py).  B, the fp64 restatement over the
oracle's lists, on the twelve depth_scenes where no rule is near its threshold (tests/test_depth_grad_boundary.py
asserts that): the image within IMG_SHARP max(1, max |f|) per element, the gradients within the same bar.
"""
import math

import numpy as np
import pytest
import torch

import alpha_scenes as AS
import depth_scenes as DS
import feature_refs as FR
import importance_refs as IR
from gpu_helpers import c_backward, to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}
A_SCENES = ["small0", "hi0", "dense0", "cov3D5", "opaque", "sparse", "sparse_culled", "stack", "wide"]
FP64_SCENES = ["small0", "small1", "small2", "small3", "hi0", "rot0", "dense0", "dense1", "dense2", "dense3",
               "colors4", "cov3D5"]


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def K():
    return int(_C().FEATURE_CHUNK)


def _scene(name):
    if name == "stack":
        return dict(s=IR.stack_scene(), colors=None, cov3D=None, use_sh=True)
    if name == "wide":
        return dict(s=IR.wide_scene(), colors=None, cov3D=None, use_sh=True)
    if name == "sparse_culled":
        return dict(s=IR.sparse_culled_scene(), colors=None, cov3D=None, use_sh=True)
    return AS.scene(name) if name in AS.NAMES else DS.scene(name)


def gpu(name, aa=False):
    """device tensors and the HIP forward of a scene (its own colours), made once"""
    key = (name, aa)
    if key not in _GPU:
        sc = _scene(name)
        d = to_dev(sc["s"], torch.device(DEV))
        colors = None if sc["colors"] is None else torch.tensor(sc["colors"], device=DEV)
        cov3D = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=DEV)
        fwd = FR.plain_forward(_C(), sc["s"], d, colors=colors, cov3D=cov3D, use_sh=sc["use_sh"], aa=aa)
        _GPU[key] = dict(sc=sc, s=sc["s"], d=d, colors=colors, cov3D=cov3D, fwd=fwd)
    return _GPU[key]


def _feats(P, C, seed, zero_column=None):
    return torch.tensor(FR.features_of(P, C, seed, zero_column), device=DEV)


def _brightest_pixel(g):
    s = g["s"]
    alpha = _C().alpha_image(g["fwd"][6], int(s["H"]), int(s["W"])).reshape(int(s["H"]), int(s["W"]))
    i = int(alpha.argmax())
    return i // int(s["W"]), i % int(s["W"])


# ---- 1. forward, exact against the composition ---------------------------------------------------------------------
@pytest.mark.parametrize("name", A_SCENES)
def test_forward_is_the_composition_bit_for_bit(name):
    g = gpu(name)
    s, P = g["s"], len(g["s"]["means3D"])
    k = K()
    for C in (1, 2, 3, k - 1, k, k + 1, 2 * k + 1):
        f = _feats(P, C, 100 + C, zero_column=k if C == 2 * k + 1 else None)
        got = FR.fused_forward(_C(), s, g["fwd"], f)
        want, _ = FR.composition_forward(_C(), s, g["d"], f, cov3D=g["cov3D"])
        assert tuple(got.shape) == (C, int(s["H"]), int(s["W"])) and got.dtype == torch.float32
        for c in range(C):
            assert torch.equal(got[c], want[c]), f"{name}: channel {c} of {C}"
        if C == 2 * k + 1:
            assert not bool(got[k].any()) and bool((got < 0).any()) and bool((got > 0).any())
    if name == "stack":  # every sort path ran and a pixel retired inside the 513 run
        lists = _C().debug_tile_lists(g["fwd"][4], g["fwd"][5], g["fwd"][6], P, int(s["W"]), int(s["H"]), g["fwd"][0])
        ranges = lists[0].cpu().numpy().astype(np.int64)
        assert (ranges[:, 1] - ranges[:, 0]).tolist() == IR.STACK_LENGTHS


# ---- 2. forward against the fp64 restatement ------------------------------------------------------------------------
_REF_B = {}


def reference_b(oracle, name):
    if name not in _REF_B:
        sc = DS.scene(name)
        ref = DS.reference(oracle, name)
        _REF_B[name] = FR.restatement(sc["s"], ref["export"]["point_list"], ref["export"]["ranges"])
    return _REF_B[name]


@pytest.mark.parametrize("name", FP64_SCENES)
def test_forward_matches_the_fp64_restatement(oracle, name):
    g = gpu(name)
    P = len(g["s"]["means3D"])
    C = K() + 1
    f = FR.features_of(P, C, 200)
    got = FR.fused_forward(_C(), g["s"], g["fwd"], torch.tensor(f, device=DEV)).double().cpu()
    r = reference_b(oracle, name)  # (the graph is built once, with gradients, for the backward tests too)
    want = FR.features_image(r, torch.tensor(f, dtype=torch.float64)).detach()
    bar = PAR.IMG_SHARP * max(1.0, float(np.abs(f).max()))
    err = float((got - want).abs().max())
    print(f"\n[features] {name}: image within {err / bar:.3f} of IMG_SHARP max(1, max|f|) of the fp64 restatement")
    assert float(want.abs().max()) > 0.05 and err <= bar


# ---- 3. backward ----------------------------------------------------------------------------------------------------
def _check_grads(tag, got, ref, cov3D):
    """every element of every gradient within the bar; returns the largest fraction of the bar used"""
    gf, m2, op, m3, dcov, dsc, drot = (t.double().cpu().numpy() for t in got)
    pairs = [("features", gf, ref["features"]), ("means2D", m2[:, :2], np.asarray(ref["means2D"])[:, :2]),
             ("opacities", op, ref["opacities"]), ("means3D", m3, ref["means3D"])]
    if cov3D:
        pairs.append(("cov3D", dcov, ref["cov3D"]))
    else:
        pairs += [("scales", dsc, ref["scales"]), ("rotations", drot, ref["rotations"])]
    worst = 0.0
    for k, a, b in pairs:
        assert a.shape == np.asarray(b).shape, (tag, k, a.shape, np.asarray(b).shape)
        used = FR.used_of_bar(a, b)
        print(f"[features] {tag}: {k} uses {used:.3f} of its bar")
        assert used <= 1.0, f"{tag}: {k} is off by {used:.3f} of GRAD_RTOL |ref| + GRAD_FLOOR max |ref|"
        worst = max(worst, used)
    assert bool((m2[:, 2:] == 0).all())
    return worst


def _upstreams(g, C, seed):
    s = g["s"]
    H, W = int(s["H"]), int(s["W"])
    y, x = _brightest_pixel(g)
    return [("normal", FR.upstream_normal(C, H, W, seed)), ("one pixel", FR.upstream_one_pixel(C, H, W, y, x))]


@pytest.mark.parametrize("name", A_SCENES)
def test_backward_matches_the_composition(name):
    g = gpu(name)
    s, P, k = g["s"], len(g["s"]["means3D"]), K()
    worst = 0.0
    for C in (1, 3, k + 1, 2 * k + 1):
        f = _feats(P, C, 300 + C)
        for kind, up in _upstreams(g, C, 400 + C):
            grad = torch.tensor(up, device=DEV)
            got = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad, cov3D=g["cov3D"])
            ref = FR.composition_backward(_C(), s, g["d"], f, grad, cov3D=g["cov3D"])
            worst = max(worst, _check_grads(f"{name} C={C} {kind} vs A", got, ref, g["cov3D"] is not None))
            if kind == "normal" and name != "sparse_culled":
                assert np.abs(ref["means3D"]).max() > 0 and np.abs(ref["features"]).max() > 0
    print(f"\n[features] {name}: backward against the composition uses at most {worst:.3f} of the bar")


@pytest.mark.parametrize("name", FP64_SCENES)
def test_backward_matches_the_fp64_restatement(oracle, name):
    g = gpu(name)
    s, P, k = g["s"], len(g["s"]["means3D"]), K()
    r = reference_b(oracle, name)
    cov = g["cov3D"] is not None
    if cov:  # the restatement's covariance leaf: the same rows the GPU takes
        r = FR.restatement(s, DS.reference(oracle, name)["export"]["point_list"],
                           DS.reference(oracle, name)["export"]["ranges"], cov3D=g["sc"]["cov3D"])
    worst = 0.0
    for C in (1, 3, k + 1, 2 * k + 1):
        fn = FR.features_of(P, C, 500 + C)
        for kind, up in _upstreams(g, C, 600 + C):
            got = FR.fused_backward(_C(), s, g["d"], g["fwd"], torch.tensor(fn, device=DEV),
                                    torch.tensor(up, device=DEV), cov3D=g["cov3D"])
            ref = FR.restatement_grads(r, torch.tensor(fn, dtype=torch.float64, requires_grad=True), up)
            worst = max(worst, _check_grads(f"{name} C={C} {kind} vs B", got, ref, cov))
    print(f"\n[features] {name}: backward against the fp64 restatement uses at most {worst:.3f} of the bar")


def test_features_only_backward_skips_the_geometry():
    g = gpu("dense0")
    s, P, C = g["s"], len(g["s"]["means3D"]), K() + 1
    f = _feats(P, C, 700)
    grad = torch.tensor(FR.upstream_normal(C, int(s["H"]), int(s["W"]), 701), device=DEV)
    full = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad)
    only = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad, geometry=False)
    assert torch.equal(only[0], full[0]) and float(full[0].abs().max()) > 0
    assert all(t.shape[0] == 0 for t in only[1:]) and all(t.shape[0] == P for t in full[1:])


# ---- 4. repeatable and inert ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense0", "opaque", "stack"])
def test_two_calls_give_the_same_bits_and_change_nothing(name):
    g = gpu(name)
    s, P, C = g["s"], len(g["s"]["means3D"]), 2 * K() + 1
    f = _feats(P, C, 800)
    grad = torch.tensor(FR.upstream_normal(C, int(s["H"]), int(s["W"]), 801), device=DEV)
    before = [t.clone() for t in g["fwd"][1:]]
    a, b = FR.fused_forward(_C(), s, g["fwd"], f), FR.fused_forward(_C(), s, g["fwd"], f)
    assert torch.equal(a, b)
    ga = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad, cov3D=g["cov3D"])
    gb = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad, cov3D=g["cov3D"])
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    for x, y in zip(before, g["fwd"][1:]):  # colour, depth, radii and the three state buffers
        assert torch.equal(x, y)


def test_a_colour_backward_after_the_pass_is_the_backward_without_it():
    sc = _scene("dense0")
    s = sc["s"]
    d = to_dev(s, torch.device(DEV))
    grad = torch.tensor(np.random.default_rng(5).normal(0, 1, (3, s["H"], s["W"])).astype(np.float32), device=DEV)
    plain = FR.plain_forward(_C(), s, d)
    want = c_backward(_C(), s, d, plain, grad)
    fwd = FR.plain_forward(_C(), s, d)
    f = _feats(len(s["means3D"]), 5, 900)
    FR.fused_forward(_C(), s, fwd, f)
    FR.fused_backward(_C(), s, d, fwd, f, torch.tensor(FR.upstream_normal(5, s["H"], s["W"], 901), device=DEV))
    got = c_backward(_C(), s, d, fwd, grad)
    for n, x, y in zip(PAR.GRAD_NAMES, got, want):
        assert torch.equal(x, y), n
    assert float(want[3].abs().max()) > 0


# ---- 5. the Python surface: outputs, composition with the options, edges --------------------------------------------
def _module_inputs(name):
    import diff_gaussian_rasterization as dgr
    g = gpu(name)
    s, d = g["s"], g["d"]
    st = dgr.GaussianRasterizationSettings(int(s["H"]), int(s["W"]), float(s["tanfovx"]), float(s["tanfovy"]), d["bg"],
                                           float(s["scale_modifier"]), d["viewmatrix"], d["projmatrix"],
                                           int(s["sh_degree"]), d["campos"], False, False)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    leaves["means2D"] = torch.zeros_like(d["means3D"]).requires_grad_(True)
    return dgr, st, leaves


def _run(dgr, st, lv, features=None, **opts):
    return dgr.GaussianRasterizer(st, **opts)(means3D=lv["means3D"], means2D=lv["means2D"], opacities=lv["opacities"],
                                              shs=lv["shs"], scales=lv["scales"], rotations=lv["rotations"],
                                              **({} if features is None else {"features": features}))


def test_the_other_outputs_keep_their_bits():
    dgr, st, lv = _module_inputs("dense0")
    P = lv["means3D"].shape[0]
    f = _feats(P, K() + 1, 1000)
    plain = _run(dgr, st, lv, alpha=True)
    out = _run(dgr, st, lv, features=f, alpha=True)
    assert len(out) == 5 and len(plain) == 4
    for x, y in zip(plain, out[:4]):
        assert torch.equal(x, y)
    want = FR.fused_forward(_C(), gpu("dense0")["s"], gpu("dense0")["fwd"], f)
    assert torch.equal(out[4], want)
    assert not out[4].requires_grad or out[4].grad_fn is not None


def test_composes_with_depth_alpha_and_absgrad():
    """losses on colour, depth, alpha and features together: each gradient is the options-only call's plus the
    features-only call's, within the bar of their sum; means2D.absgrad is the options-only call's bits"""
    dgr, st, _ = _module_inputs("dense0")
    s = gpu("dense0")["s"]
    H, W, P, C = int(s["H"]), int(s["W"]), len(s["means3D"]), K() + 1
    rng = np.random.default_rng(1100)
    t = lambda *shape: torch.tensor(rng.normal(0, 1, shape).astype(np.float32), device=DEV)
    g_c, g_d, g_a, g_f = t(3, H, W), t(1, H, W), t(1, H, W), t(C, H, W)
    f0 = FR.features_of(P, C, 1101)
    opts = dict(alpha=True, depth_grad=True, absgrad=True)

    def grads(use_options, use_features):
        _, _, lv = _module_inputs("dense0")
        f = torch.tensor(f0, device=DEV, requires_grad=True)
        out = _run(dgr, st, lv, features=f if use_features else None, **opts)
        loss = 0
        if use_options:
            loss = loss + (out[0] * g_c).sum() + (out[2] * g_d).sum() + (out[3] * g_a).sum()
        if use_features:
            loss = loss + (out[-1] * g_f).sum()
        loss.backward()
        res = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in lv.items()}
        res["features"] = f.grad
        res["absgrad"] = getattr(lv["means2D"], "absgrad", None)
        return res
    both, opt_only, feat_only = grads(True, True), grads(True, False), grads(False, True)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        want = opt_only[k].double().cpu().numpy() + feat_only[k].double().cpu().numpy()
        used = FR.used_of_bar(both[k].double().cpu().numpy(), want)
        assert used <= 1.0, (k, used)
    assert torch.equal(both["features"], feat_only["features"]) and opt_only["features"] is None
    assert torch.equal(both["absgrad"], opt_only["absgrad"]) and float(both["absgrad"].abs().max()) > 0
    assert float(feat_only["means3D"].abs().max()) > 0 and not bool(feat_only["shs"].any())


def test_antialiased_features_are_the_antialiased_composition():
    g, ga = gpu("small0"), gpu("small0", aa=True)
    s, P, C = g["s"], len(g["s"]["means3D"]), K() + 1
    f = _feats(P, C, 1200)
    got = FR.fused_forward(_C(), s, ga["fwd"], f)
    want, _ = FR.composition_forward(_C(), s, ga["d"], f, aa=True)
    assert torch.equal(got, want) and not torch.equal(got, FR.fused_forward(_C(), s, g["fwd"], f))
    grad = torch.tensor(FR.upstream_normal(C, int(s["H"]), int(s["W"]), 1201), device=DEV)
    back = FR.fused_backward(_C(), s, ga["d"], ga["fwd"], f, grad, aa=True)
    ref = FR.composition_backward(_C(), s, ga["d"], f, grad, aa=True)
    _check_grads("small0 antialiased vs A", back, ref, False)
    plain = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, grad)
    assert not torch.equal(plain[2], back[2])


def test_edges():
    import diff_gaussian_rasterization as dgr
    # P = 0: a zero image, and a backward that gives an empty gradient
    _, st, _ = _module_inputs("dense0")
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    f = z(0, 4).requires_grad_(True)
    out = dgr.GaussianRasterizer(st)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 16, 3),
                                     scales=z(0, 3), rotations=z(0, 4), features=f)
    assert tuple(out[3].shape) == (4, st.image_height, st.image_width) and not bool(out[3].any())
    out[3].sum().backward()
    assert tuple(f.grad.shape) == (0, 4)
    # a view that culls everything
    g = gpu("behind")
    s, P = g["s"], len(g["s"]["means3D"])
    assert g["fwd"][0] == 0
    f = _feats(P, 3, 1300)
    img = FR.fused_forward(_C(), s, g["fwd"], f)
    assert tuple(img.shape) == (3, int(s["H"]), int(s["W"])) and not bool(img.any())
    back = FR.fused_backward(_C(), s, g["d"], g["fwd"], f, torch.ones_like(img))
    assert all(tuple(t.shape)[0] == P and not bool(t.any()) for t in back)
    # features that do not require grad receive none; the geometry still does
    dgr, st, lv = _module_inputs("dense0")
    f = _feats(lv["means3D"].shape[0], 3, 1301)
    out = _run(dgr, st, lv, features=f)
    out[3].square().sum().backward()
    assert f.grad is None and float(lv["means3D"].grad.abs().max()) > 0
    # features alone require grad: the geometry receives none
    _, _, lv2 = _module_inputs("dense0")
    for v in lv2.values():
        v.requires_grad_(False)
    f2 = f.clone().requires_grad_(True)
    _run(dgr, st, lv2, features=f2)[3].square().sum().backward()
    assert float(f2.grad.abs().max()) > 0 and all(v.grad is None for v in lv2.values())
    with pytest.raises(ValueError):
        _run(dgr, st, lv, features=f, camera_grad=True)


# ---- 6. stream -------------------------------------------------------------------------------------------------------
def test_the_passes_on_a_side_stream():
    """tests/test_streams_gpu.py's pattern through its harness with a case of this file's own: the forward, the feature
    pass and its backward queued on a side stream behind delayed copies of the inputs, with the null stream blocked,
    give the default stream's bits"""
    import stream_cases as SC
    C = K() + 1

    def make(seed):
        t = SC.raster_inputs(seed)
        rng = np.random.default_rng(seed + 500)
        t["features"] = torch.tensor(rng.normal(0, 1, (SC.RASTER["P"], C)).astype(np.float32))
        t["g_features"] = torch.tensor(rng.normal(0, 1, (C, SC.RASTER["H"], SC.RASTER["W"])).astype(np.float32))
        return t

    def call(t):
        fwd = SC.raster_forward(t)
        tx, ty, sm = SC._raster_consts()
        e = torch.empty(0, device=t["means3D"].device)
        img = _C().rasterize_features(t["features"], fwd[4], fwd[0], fwd[5], fwd[6], SC.RASTER["P"], SC.RASTER["H"],
                                      SC.RASTER["W"])
        back = _C().rasterize_features_backward(t["features"], t["g_features"], t["means3D"], fwd[3], t["scales"],
                                                t["rotations"], sm, e, t["viewmatrix"], t["projmatrix"], tx, ty, fwd[4],
                                                fwd[0], fwd[5], fwd[6], e, False, True)
        return [img] + list(back)
    case = SC.Case("rasterize_features", ["rasterize_features", "rasterize_features_backward"], make, call)
    host, want = SC.run_case(case, SC.calibration(DEV).fresh_stream())
    assert len(host) == 8 and float(host[0].abs().sum()) > 0 and float(host[4].abs().sum()) > 0


# ---- 7. render, render_view, render_flow -----------------------------------------------------------------------------
def _model():
    if "model" not in _GPU:
        _GPU["model"] = FR.model_and_views()
    return _GPU["model"]


def test_render_carries_the_features():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import infer
    from gs4d_train.render import render
    g, cams, _, _ = _model()
    cam, bg = cams[1], torch.ones(3, device="cuda")
    P = g.get_xyz.shape[0]
    f = _feats(P, 5, 1400)
    seen = []

    def rows(m3):
        seen.append(m3)
        return f
    with torch.no_grad():
        plain = render(cam, g, False, bg)
        pkg = render(cam, g, False, bg, features=f)
        pkg2 = render(cam, g, False, bg, features=rows)
    assert "features" not in plain and tuple(pkg["features"].shape) == (5, 48, 64)
    assert torch.equal(pkg["render"], plain["render"]) and torch.equal(pkg["features"], pkg2["features"])
    # the callable received the deformed means: the rasterizer called by hand on them gives the image
    assert len(seen) == 1 and tuple(seen[0].shape) == (P, 3) and not torch.equal(seen[0], g.get_xyz)
    state = infer.prepare(g)
    st = infer._raster_settings(cam, state, bg)
    m3, sc, rot, op, sh = infer.state_at_time(state, cam.time)
    hand = dgr.GaussianRasterizer(st)(means3D=m3, means2D=torch.zeros_like(m3), opacities=op, shs=sh, scales=sc,
                                      rotations=rot, features=f)
    view = infer.render_view(cam, state, bg, features=f)
    assert torch.equal(view["features"], hand[3]) and torch.equal(view["render"], hand[0])
    # render()'s fine-stage image: render_view's fused deformation is not render()'s bit for bit, so the bar is the one
    # tests/test_infer_gpu.py holds that pair to: mean |render_view - unfused render()| <= 2 d0 + 1e-6, d0 = mean |fused
    # render() - unfused render()|
    net = g._deformation.deformation_net
    try:
        with torch.no_grad():
            g.fused = net.grid.fused = net.fused_heads = False
            unfused = render(cam, g, False, bg, features=f)["features"]
    finally:
        g.fused = net.grid.fused = net.fused_heads = True
    d0 = float((pkg["features"] - unfused).abs().mean())
    d1 = float((view["features"] - unfused).abs().mean())
    print(f"\n[features] render_view fine stage: mean |render_view - unfused render()| = {d1:.3e}, d0 = {d0:.3e}")
    assert d1 <= 2 * d0 + 1e-6
    # render()'s own image, bit for bit, where the two paths share their kernels: the coarse stage
    with torch.no_grad():
        coarse = render(cam, g, False, bg, stage="coarse", features=f)
    cview = infer.render_view(cam, infer.prepare(g, stage="coarse"), bg, features=f)
    assert torch.equal(cview["features"], coarse["features"]) and float(coarse["features"].abs().max()) > 0


def _hand_flow_rows(g, cam, dt):
    """The flow rows written out by hand: the deformation module called at the two times, the rasterizer's pixel
    mapping through the camera's full projection, the view-depth rule -- nothing of gs4d_train.flow.  Returns
    (rows (P, 2) float32 with a graph, behind (P,) bool, bound (P, 2) float64, depth at t + dt (P,) float64, front
    (P,) bool = in front of the near plane at both times).

    bound: how far two correct float32 evaluations of a row may lie apart.  pix_a = ((x_a / w + 1) S_a - 1) / 2 with
    (x, ., ., w) = (m, 1) @ proj, so an error d in the position moves pix_a by at most
    (S_a / 2) (|proj[:3, a]|_1 + |ndc_a| |proj[:3, 3]|_1) |d|_inf / |w|.  Two float32 paths through the same MLP and
    field (render()'s fused heads against the plain layers) agree to EPS_POS = 1e-5 max(1, A) in the position, A the
    largest displacement the deformation gives a coordinate here (sums of up to 256 products of values of order A:
    256 x 2^-24 x a few, taken ten times over); each path's own evaluation of pix adds
    8 u (S_a / 2) (sum of |terms| of x_a + |ndc_a| sum of |terms| of w) / |w| + 4 u (|pix_a| + S_a), u = 2^-24.  A row is
    the difference of two such values."""
    U = 2.0 ** -24
    xyz = g.get_xyz
    P, dev = xyz.shape[0], xyz.device
    W, H = int(cam.image_width), int(cam.image_height)
    proj, view = cam.full_proj_transform.to(dev), cam.world_view_transform.to(dev)
    size = torch.tensor([float(W), float(H)], device=dev)
    t0 = float(np.float32(cam.time))
    t1 = float(np.float32(t0 + dt))

    def means(t):
        time = torch.full((P, 1), t, dtype=torch.float32, device=dev)
        return g._deformation(xyz, g._scaling, g._rotation, g._opacity, g.get_features, time)[0]

    def pix(m):
        hom = torch.cat([m, torch.ones_like(m[:, :1])], 1) @ proj
        ndc = hom[:, :2] / (hom[:, 3:4] + 0.0000001)
        return ((ndc + 1.0) * size - 1.0) / 2.0

    def pix_bound(m):
        m, pr, sz = m.detach().double(), proj.double(), size.double()
        hom = torch.cat([m, torch.ones_like(m[:, :1])], 1) @ pr
        w = hom[:, 3:4].abs()
        ndc = (hom[:, :2] / hom[:, 3:4]).abs()
        col1 = pr[:3, :2].abs().sum(0, keepdim=True)                      # |proj[:3, a]|_1
        w1 = pr[:3, 3].abs().sum()
        terms = torch.cat([m.abs(), torch.ones_like(m[:, :1])], 1) @ pr.abs()   # sum of |terms| of each component
        moved = sz / 2 * (col1 + ndc * w1) * EPS_POS / w
        rounded = 8 * U * sz / 2 * (terms[:, :2] + ndc * terms[:, 3:4]) / w + 4 * U * ((ndc + 1) * sz / 2 + sz)
        return moved + 2 * rounded
    m0, m1 = means(t0), means(t1)
    A = max(float((m0.detach() - xyz.detach()).abs().max()), float((m1.detach() - xyz.detach()).abs().max()))
    EPS_POS = 1e-5 * max(1.0, A)
    depth1 = torch.cat([m1, torch.ones_like(m1[:, :1])], 1) @ view[:, 2]
    behind = depth1 <= 0.2
    rows = torch.where(behind.unsqueeze(1), torch.zeros_like(m0[:, :2]), pix(m1) - pix(m0))
    depth0 = torch.cat([m0, torch.ones_like(m0[:, :1])], 1) @ view[:, 2]
    return rows, behind, pix_bound(m0) + pix_bound(m1), depth1.detach().double(), (~behind & (depth0 > 0.2)).detach()


def _check_flow_against_hand(g, cam, bg, dt, tag):
    from gs4d_train.flow import flow_rows, render_flow
    from gs4d_train.render import render
    rows, behind, bound, depth1, ok = _hand_flow_rows(g, cam, dt)
    assert not bool(((depth1 - 0.2).abs() < 1e-4).any())  # no Gaussian whose depth rule rounding could decide
    seen = []
    pkg = render_flow(cam, g, bg, dt)
    hand = render(cam, g, False, bg, features=lambda m3: seen.append(m3) or rows)
    got_rows = flow_rows(cam, g, seen[0], dt).detach()
    assert not bool(got_rows[behind].any())  # exactly zero behind the camera at t + dt
    err = (got_rows.double() - rows.detach().double()).abs()[ok]
    used = float((err / bound[ok]).max())
    drawn = (hand["radii"] > 0) & ok
    n_list = 1024  # longer than any tile list of this scene (600 Gaussians)
    tol = float(bound[drawn].max()) + 2 * n_list * 2.0 ** -24 * float(rows.detach().abs()[drawn].max())
    diff = float((pkg["flow"].detach() - hand["features"].detach()).abs().max())
    peak = float(hand["features"].detach().abs().max())
    print(f"\n[features] flow {tag}: rows within {used:.3f} of their bound; image differs by {diff:.3e} (bar {tol:.3e}), "
          f"largest flow {peak:.3f} px; {int(behind.sum())} Gaussians behind the camera at t + dt")
    assert used <= 1.0 and diff <= tol and peak > 10 * tol
    assert torch.equal(pkg["render"], hand["render"])
    return pkg, behind, hand


def test_render_flow():
    """render_flow against the composition written out by hand (_hand_flow_rows: two calls of the deformation module,
    the pixel mapping and the depth rule in the test's own code) fed through render(features=...): the rows within
    the bound derived there, the image within the largest bound of a drawn Gaussian plus the blend's rounding.  Two
    cameras: a view of the scene, and one placed so that a chosen Gaussian is in front of it at t (drawn) and behind
    its near plane at t + dt, whose row must be exactly zero."""
    from gs4d_train.flow import render_flow
    from gs4d_train.synthetic import look_at_camera
    if "flow_model" not in _GPU:
        # the position head scaled: the re-drawn network moves a point by about 2e-4 over dt (a few 1e-3 pixels) on
        # top of an offset of about 0.03 common to all points; times 30 the motion is tenths of a pixel and the
        # offset, about one unit, leaves the scene in view
        _GPU["flow_model"] = FR.model_and_views(motion=30.0)
    g, cams, _, _ = _GPU["flow_model"]
    cam, bg, dt = cams[1], torch.ones(3, device="cuda"), 0.1
    with torch.no_grad():
        coarse = render_flow(cam, g, bg, dt, stage="coarse")
    assert tuple(coarse["flow"].shape) == (2, 48, 64) and not bool(coarse["flow"].any()) and "features" not in coarse
    for p in g._deformation.parameters():
        p.grad = None
    pkg, behind, _ = _check_flow_against_hand(g, cam, bg, dt, "view 1")
    assert float(pkg["flow"].detach().abs().max()) > 1e-3  # the perturbed network moves the points
    pkg["flow"].square().sum().backward()
    grads = [p.grad for p in g._deformation.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    # the second camera: Gaussian i moves from m_t to m_dt; the eye sits on that line, looking along m_dt -> m_t from
    # 0.2 in front of the midpoint, so the view depths are 0.2 + |m_t - m_dt| / 2 at t and 0.2 - |m_t - m_dt| / 2 at t + dt
    xyz = g.get_xyz
    P = xyz.shape[0]
    with torch.no_grad():
        at = lambda t: g._deformation(xyz, g._scaling, g._rotation, g._opacity, g.get_features,
                                      torch.full((P, 1), t, dtype=torch.float32, device=xyz.device))[0].double().cpu().numpy()
        t0 = float(np.float32(cam.time))
        m_t, m_dt = at(t0), at(float(np.float32(t0 + dt)))
    step = np.linalg.norm(m_t - m_dt, axis=1)
    u = (m_t - m_dt) / np.maximum(step, 1e-30)[:, None]
    step[np.abs(u[:, 1]) > 0.9] = 0  # look_at_camera's up vector is y
    i = int(step.argmax())
    assert step[i] > 1e-3
    eye = 0.5 * (m_t[i] + m_dt[i]) - 0.2 * u[i]
    cam2 = look_at_camera(64, 48, tuple(eye), target=tuple(eye + u[i]), time=cam.time)
    pkg2, behind2, hand2 = _check_flow_against_hand(g, cam2, bg, dt, "near-plane view")
    assert bool(behind2[i]) and int(hand2["radii"][i]) > 0  # drawn at t, behind the near plane at t + dt
    with pytest.raises(ValueError):
        render_flow(cam, g, bg, dt, features=torch.zeros(1, 1))
