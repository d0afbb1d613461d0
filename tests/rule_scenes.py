"""Scenes on which the rasterizer's rule-bound branches run, and their fp64 references (test infrastructure).

The scenes of tests/depth_scenes.py keep every non-differentiable rule of the reference inactive.  These make each
one bind, far enough from its threshold (tests/test_rule_branches_boundary.py asserts the margins) that every
element is still compared with the fp64 restatement (tests/torch_restatement.py), which restates the rules as the
reference's backward treats them:

  clamp        P=80, 70x45, a rotated, translated camera with fovx = 60 deg and an INDEPENDENT fovy = 35 deg
               (focal_x ~ 60.6, focal_y ~ 71.4), view positions out to 1.7 tan_fov: a quarter of the visible
               Gaussians lie beyond the 1.3 tan_fov frustum clamp of computeCov2D (Q22) and still overlap the image
  clampmod     clamp with scale_modifier = 0.7 (Q26)
  indef_dense  depth_scenes' dense scene (P=300, 40x24, lists of 100-230) through cov3D_precomp, every k-th
               Gaussian's second squared scale negated: conics that are not positive definite, whose power > 0
               pairs are skipped.  k = 5 puts one in nearly every 64-splat batch, k = 29 leaves full batches
               with and without one (the blend kernels' folded and general walks)
  indef_small  depth_scenes' small scene with k = 4: lists shorter than one batch
  term         P=200, 70x45, large splats of opacity 0.55-0.95 with every 5th at 0.999: the 0.99 cap binds (Q17),
               pixels terminate, lists hold several batches
  *_colors     one clamp and one indef_small scene with colors_precomp

Same shape as depth_scenes (ENTRIES, scene, reference, upstream, autograd_grads), with an alpha term in the loss:
sum(color * g_c) + sum(depth * g_d) + sum((1 - Tfinal) * g_A).  These scenes are NOT in depth_scenes.ENTRIES: the
depth, alpha and absgrad suites measure their floor over that list.
"""
import math

import numpy as np
import torch

import depth_scenes as DS
from gs4d_train.camera import Camera
from gs4d_train.synthetic import make_scene, make_upstream_grad


def view_with_camera(s, fovx_deg=60.0, fovy_deg=35.0, rescale_y=True):
    """The scene seen by a rotated, translated camera (R, T of depth_scenes._rot) whose fovy does not follow from fovx
    and the aspect ratio, the means moved to world space so that their view coordinates stay (rescale_y: y is first
    rescaled to the new tan_fovy, so a spread in units of tan_fov is kept)."""
    cy, sy, cx, sx = math.cos(0.4), math.sin(0.4), math.cos(-0.3), math.sin(-0.3)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R, T = Ry @ Rx, np.array([0.3, -0.2, 0.5])
    cam = Camera(R, T, math.radians(fovx_deg), math.radians(fovy_deg), s["W"], s["H"])
    view = s["means3D"].astype(np.float64)
    if rescale_y:
        view[:, 1] *= cam.tanfovy / s["tanfovy"]
    # p_view = R^T p_world + T (the reference's getWorld2View2), so p_world = R (p_view - T)
    s["means3D"] = ((view - T) @ R.T).astype(np.float32)
    s["viewmatrix"] = cam.world_view_transform.numpy().astype(np.float32)
    s["projmatrix"] = cam.full_proj_transform.numpy().astype(np.float32)
    s["campos"] = cam.camera_center.numpy().astype(np.float32)
    s["tanfovx"], s["tanfovy"] = cam.tanfovx, cam.tanfovy
    s["camera"] = cam
    return s


def _clamp(seed):
    s = make_scene(80, 70, 45, seed=seed, sh_degree=3, spread=1.7, log_scale=math.log(0.25), z_range=(2.0, 6.0))
    s["opacities"] = (0.5 * np.minimum(s["opacities"], 0.6)).astype(np.float32)
    return view_with_camera(s)


def _clampmod(seed):
    s = _clamp(seed)
    s["scale_modifier"] = 0.7
    return s


def _term(seed):
    s = make_scene(200, 70, 45, seed=seed, sh_degree=3, log_scale=math.log(0.2), z_range=(2.0, 6.0))
    s["opacities"] = (0.55 + 0.4 * np.random.default_rng(seed + 9).uniform(0, 1, (200, 1))).astype(np.float32)
    s["opacities"][::5] = 0.999
    return s


def indefinite_cov3d(s, k):
    """cov3D_precomp rows of the scene's scales and rotations with every k-th Gaussian's second squared scale
    negated: a symmetric matrix with one negative eigenvalue"""
    from torch_restatement import quat_to_rot
    R = quat_to_rot(torch.tensor(s["rotations"], dtype=torch.float64)).numpy()
    S2 = s["scales"].astype(np.float64) ** 2
    S2[::k, 1] *= -1.0
    C = np.einsum("pij,pj,pkj->pik", R, S2, R)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1).astype(np.float32)


# seeds: the first ones on which every condition of tests/test_rule_branches_boundary.py holds (a seed with a
# decision inside a flip band or a margin is passed over, never the condition).  clamp seed 2 has a Gaussian 5.6e-5
# from the clamp limit; indef_dense k = 5 seeds 0-8 have a power-sign margin below 1e-4, a flip flag or a
# non-positive-definite conic that contributes nowhere.  indef_small: the power of an indefinite conic is a
# difference of large terms, and on these small, sharp splats the fp32 oracle's colour is 4e-6 to 2.6e-5 from fp64 on
# seeds 0-79 except 33, where it meets the 2e-6 bar of tests/test_oracle.py.
ENTRIES = [
    dict(name="clamp1", make=_clamp, seed=1, mode="sh", k=0),
    dict(name="clamp3", make=_clamp, seed=3, mode="sh", k=0),
    dict(name="clampmod7", make=_clampmod, seed=7, mode="sh", k=0),
    dict(name="clamp_colors4", make=_clamp, seed=4, mode="colors", k=0),
    dict(name="indef_dense_k5", make=DS._dense, seed=9, mode="cov3D", k=5),
    dict(name="indef_dense_k29", make=DS._dense, seed=0, mode="cov3D", k=29),
    dict(name="indef_small", make=DS._small, seed=33, mode="cov3D", k=4),
    dict(name="indef_small_colors", make=DS._small, seed=33, mode="cov3D+colors", k=4),
    dict(name="term2", make=_term, seed=2, mode="sh", k=0),
    dict(name="term3", make=_term, seed=3, mode="sh", k=0),
]
NAMES = [e["name"] for e in ENTRIES]
_CACHE = {}


def build(e):
    """depth_scenes.scene's dict for an entry (also used to look for seeds)"""
    s = e["make"](e["seed"])
    colors = cov3D = None
    if "colors" in e["mode"]:
        colors = np.random.default_rng(e["seed"] + 100).uniform(0, 1, (s["means3D"].shape[0], 3)).astype(np.float32)
    if "cov3D" in e["mode"]:
        cov3D = indefinite_cov3d(s, e["k"])
    return dict(name=e["name"], s=s, colors=colors, cov3D=cov3D, use_sh=colors is None, mode=e["mode"], k=e["k"])


def scene(name):
    """The scene `name`: dict(s=make_scene's dict, colors / cov3D = the precomputed inputs or None, use_sh, mode)."""
    if name not in _CACHE:
        _CACHE[name] = build(ENTRIES[NAMES.index(name)])
    return _CACHE[name]


_REF = {}


def make_reference(O, sc):
    from gpu_helpers import o_forward
    from torch_restatement import forward_autograd
    s = sc["s"]
    nr, color, depth, radii, st = o_forward(O, s, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    ex = st.export()
    ref = forward_autograd(s, ex["point_list"], ex["ranges"], s["sh_degree"],
                           use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"])
    return dict(color=color, depth=depth, radii=radii, state=st, export=ex, ref=ref, nr=nr)


def reference(O, name):
    """The oracle's forward of the scene and the fp64 autograd forward over the oracle's sorted lists, made once
    per scene: dict(color, depth, radii, state, export, ref = forward_autograd's dict, nr)."""
    if name not in _REF:
        _REF[name] = make_reference(O, scene(name))
    return _REF[name]


def upstream(O, name, case):
    """(g_c (3, H, W), g_d (1, H, W), g_A (1, H, W)) float32.  "color": depth_scenes.upstream's colour-only gradient
    (make_upstream_grad * 3WH), g_d = g_A = 0; "both": that g_c with g_d ~ N(0, 1); "all": "both" with g_A ~ N(0, 1)."""
    assert case in ("color", "both", "all")
    s = scene(name)["s"]
    H, W = s["H"], s["W"]
    seed = ENTRIES[NAMES.index(name)]["seed"]
    g_d = np.random.default_rng(1000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_a = np.random.default_rng(2000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_c = (make_upstream_grad(reference(O, name)["color"], seed=seed + 1)[0] * (3 * W * H)).astype(np.float32)
    if case == "color":
        g_d = np.zeros_like(g_d)
    if case != "all":
        g_a = np.zeros_like(g_a)
    return g_c, g_d, g_a


def grads_of(sc, ref, g_c, g_d, g_a):
    """fp64 gradients of sum(color * g_c) + sum(depth * g_d) + sum((1 - Tfinal) * g_A), aligned with
    _C.rasterize_gaussians_backward's tuple; None where the scene's input mode has no such gradient.  dL_dscales is
    the reference's: autograd's divided by scale_modifier (Q26)."""
    precomp = ref["cov6"] is not None
    leaves = [ref["ndc_off"], ref["rgb"], ref["opac"], ref["means"], ref["cov6"] if precomp else ref["cov3"],
              ref["shs"], ref["scales"], ref["rots"]]
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    loss = (ref["color"] * f64(g_c)).sum() + (ref["depth"] * f64(g_d)).sum() + \
        ((1.0 - ref["Tfinal"]) * f64(g_a)[0]).sum()
    gr = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    z = lambda t, like: np.zeros(tuple(like.shape)) if t is None else t.numpy()
    dm2, dcol, dop, dm3, gc, dsh, dsc, drot = (z(g, l) for g, l in zip(gr, leaves))
    packed = gc if precomp else np.stack([gc[:, 0, 0], gc[:, 0, 1] + gc[:, 1, 0], gc[:, 0, 2] + gc[:, 2, 0],
                                          gc[:, 1, 1], gc[:, 1, 2] + gc[:, 2, 1], gc[:, 2, 2]], 1)
    return [dm2, dcol, dop, dm3, packed, dsh if sc["use_sh"] else None,
            None if precomp else dsc / ref["scale_modifier"], None if precomp else drot]


def autograd_grads(O, name, g_c, g_d, g_a):
    return grads_of(scene(name), reference(O, name)["ref"], g_c, g_d, g_a)


_FW = {}


def absgrad(O, name, g_c, g_d, g_a):
    """the fp64 absgrad (P, 2) of the scene (tests/absgrad_refs.py), its signed sum checked against autograd_grads'
    dL_dmeans2D"""
    import absgrad_refs as AR
    if name not in _FW:
        sc, ref = scene(name), reference(O, name)
        s = sc["s"]
        _FW[name] = AR.per_pixel_forward(s, ref["export"]["point_list"], ref["export"]["ranges"], s["sh_degree"],
                                         colors=sc["colors"], cov3D=sc["cov3D"])
    want = autograd_grads(O, name, g_c, g_d, g_a)[0]
    return AR.absgrad_reference(_FW[name], g_c, g_d, signed_want=want, g_a=g_a)[0]
