"""Scenes of the antialiased-rasterization tests and their fp64 references (test infrastructure).

Small splats at 70x45, from gs4d_train.synthetic.make_scene(..., z_range=(2.0, 6.0)), on which the opacity factor
s = sqrt(max(2.5e-5, det S / det(S + 0.3 I))) is far from 1:

  aa_small       P=200, log_scale=log(0.03): over the listed Gaussians of seed 0 s spans 0.083-0.845, median 0.426,
                 and no Gaussian is at the floor
  aa_mid         P=200, log_scale=log(0.06): s spans 0.262-0.956, median 0.741
  aa_mid_colors  aa_mid with colors_precomp
  aa_mid_cov3D   aa_mid through cov3D_precomp (dL_dcov3D is an output there)
  aa_clampcam    aa_mid's splats with spread 1.7 seen through rule_scenes.view_with_camera: the frustum clamp (Q22)
                 and the compensation bind on the same Gaussians (P=300; the clamped ones that still overlap the
                 image are the large ones)
  aa_floor       aa_mid with every 6th Gaussian's scales 5e-4 (r ~ 1e-7, far below the floor 2.5e-5), its opacity
                 0.97 and its mean moved so that it projects onto a pixel centre: 0.005 * 0.97 clears 1/255 there,
                 the floored Gaussian blends, and the dL/dr = 0 branch carries a non-zero dL/do

Same shape as rule_scenes (ENTRIES, scene, reference, upstream, autograd_grads).  The reference of a scene is the
fp64 restatement tests/antialias_refs.py over the sorted lists of the fp32 oracle, which has no antialiasing and is
run on the FOLDED plain problem: the same scene with opacities fl32(o * s), s from the fp64 restatement.  The
lists do not depend on the opacity (the oracle bins the whole 3-sigma rectangle), and the oracle's near-threshold
flags on the folded problem are the ones that matter for the antialiased one.
"""
import math

import numpy as np

import antialias_refs as AAR
import depth_scenes as DS
import rule_scenes as RS
from gs4d_train.synthetic import make_scene, make_upstream_grad

FLOOR_EVERY = 6


def _small(seed):
    return make_scene(200, 70, 45, seed=seed, sh_degree=3, log_scale=math.log(0.03), z_range=(2.0, 6.0))


def _mid(seed):
    return make_scene(200, 70, 45, seed=seed, sh_degree=3, log_scale=math.log(0.06), z_range=(2.0, 6.0))


def _clampcam(seed):
    s = make_scene(300, 70, 45, seed=seed, sh_degree=3, spread=1.7, log_scale=math.log(0.06), z_range=(2.0, 6.0))
    return RS.view_with_camera(s)


def _floor(seed):
    s = _mid(seed)
    rows = np.arange(0, s["means3D"].shape[0], FLOOR_EVERY)
    s["scales"][rows] = 5e-4
    s["opacities"][rows] = 0.97
    # identity view matrix: pixel = ((x / (z tan_fovx) + 1) W - 1) / 2, so the nearest pixel centre inside the image
    # is reached by moving x and y at the Gaussian's own depth
    m = s["means3D"].astype(np.float64)
    z = m[rows, 2]
    for axis, n, tf in ((0, s["W"], s["tanfovx"]), (1, s["H"], s["tanfovy"])):
        pix = ((m[rows, axis] / (z * tf) + 1.0) * n - 1.0) * 0.5
        pix = np.clip(np.round(pix), 2, n - 3)
        m[rows, axis] = ((2.0 * pix + 1.0) / n - 1.0) * z * tf
    s["means3D"] = m.astype(np.float32)
    return s


# seeds: the first ones on which every condition of tests/test_antialias_boundary.py holds (a seed with a decision
# inside a flip band or a margin is passed over, never the condition; at most 20 seeds are tried per scene).  Seed 0,
# the first one tried, meets them on every scene.
ENTRIES = [
    dict(name="aa_small", make=_small, seed=0, mode="sh"),
    dict(name="aa_mid", make=_mid, seed=0, mode="sh"),
    dict(name="aa_mid_colors", make=_mid, seed=0, mode="colors"),
    dict(name="aa_mid_cov3D", make=_mid, seed=0, mode="cov3D"),
    dict(name="aa_clampcam", make=_clampcam, seed=0, mode="sh"),
    dict(name="aa_floor", make=_floor, seed=0, mode="sh"),
]
NAMES = [e["name"] for e in ENTRIES]
_CACHE, _REF = {}, {}


def build(e):
    """rule_scenes.scene's dict for an entry (also used to look for seeds)"""
    s = e["make"](e["seed"])
    colors = cov3D = None
    if e["mode"] == "colors":
        colors = np.random.default_rng(e["seed"] + 100).uniform(0, 1, (s["means3D"].shape[0], 3)).astype(np.float32)
    if e["mode"] == "cov3D":
        cov3D = DS._cov3d(s)
    return dict(name=e["name"], s=s, colors=colors, cov3D=cov3D, use_sh=colors is None, mode=e["mode"], k=0)


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = build(ENTRIES[NAMES.index(name)])
    return _CACHE[name]


def make_reference(O, sc):
    """dict(fold = the folded plain scene, s64 / r64 / floored / kappa (P,), nr, color, depth, radii, state, export
    = the oracle's forward of the folded scene, ref = antialias_refs.forward_autograd's dict over its lists)"""
    from gpu_helpers import o_forward
    s = sc["s"]
    s64, r64, floored, kappa = AAR.factor(s, sc["cov3D"])
    fold = dict(s)
    fold["opacities"] = (s["opacities"].astype(np.float64) * s64[:, None]).astype(np.float32)
    nr, color, depth, radii, st = o_forward(O, fold, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    ex = st.export()
    ref = AAR.forward_autograd(s, ex["point_list"], ex["ranges"], s["sh_degree"],
                               use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"])
    return dict(fold=fold, s64=s64, r64=r64, floored=floored, kappa=kappa, nr=nr, color=color, depth=depth,
                radii=radii, state=st, export=ex, ref=ref)


def reference(O, name):
    if name not in _REF:
        _REF[name] = make_reference(O, scene(name))
    return _REF[name]


def upstream_of(color, seed, H, W, case):
    """rule_scenes.upstream's images for a colour image and a seed"""
    assert case in ("color", "both", "all")
    g_d = np.random.default_rng(1000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_a = np.random.default_rng(2000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_c = (make_upstream_grad(color, seed=seed + 1)[0] * (3 * W * H)).astype(np.float32)
    if case == "color":
        g_d = np.zeros_like(g_d)
    if case != "all":
        g_a = np.zeros_like(g_a)
    return g_c, g_d, g_a


def upstream(O, name, case):
    """(g_c (3, H, W), g_d (1, H, W), g_A (1, H, W)) float32, as rule_scenes.upstream: "color", "both" or "all" """
    s = scene(name)["s"]
    return upstream_of(reference(O, name)["color"], ENTRIES[NAMES.index(name)]["seed"], s["H"], s["W"], case)


def autograd_grads(O, name, g_c, g_d, g_a):
    """fp64 gradients of sum(color * g_c) + sum(depth * g_d) + sum((1 - Tfinal) * g_A) of the antialiased forward,
    aligned with the backward entries' tuple (rule_scenes.grads_of)"""
    return RS.grads_of(scene(name), reference(O, name)["ref"], g_c, g_d, g_a)


_FOLD = {}


def oracle_floor_pairs(O, name):
    """(oracle gradients, fp64 gradients, radii) of the FOLDED plain problem with the colour-only upstream gradient:
    what F_oracle is measured on (reference side only)"""
    if name not in _FOLD:
        from gpu_helpers import o_backward
        from torch_restatement import forward_autograd
        sc, r = scene(name), reference(O, name)
        fold, ex = r["fold"], r["export"]
        plain = forward_autograd(fold, ex["point_list"], ex["ranges"], fold["sh_degree"],
                                 use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"])
        g_c, g_d, g_a = upstream(O, name, "color")
        got = o_backward(O, fold, r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"],
                         use_sh=sc["use_sh"])
        _FOLD[name] = (got, RS.grads_of(sc, plain, g_c, g_d, g_a), r["radii"], plain)
    return _FOLD[name]
