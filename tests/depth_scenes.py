"""Scenes and fp64 references of the depth-gradient tests (test infrastructure).

Small scenes built from gs4d_train.synthetic.make_scene on which none of the blend's discrete rules is near its
threshold (asserted by tests/test_depth_grad_boundary.py), so every gradient element can be compared with the fp64
autograd restatement (tests/torch_restatement.py) of sum(color * g_c) + sum(depth * g_d):

  small  P=60, 70x45 (no multiple of 16), short tile lists, opacities capped at 0.9; seeds 0-3
  hi     small with every 4th opacity 0.985: above 0.98 the backward takes its general (cap-capable) walk, and
         the 0.99 cap still never binds
  rot    small seen by a rotated, translated camera, the means moved so that their view coordinates stay: an
         identity view matrix cannot tell the depth row from any other
  dense  P=300, 40x24, large faint splats: tile lists of 77-239 (several 64-splat batches, odd lengths)
  modes  small seed 4 with colors_precomp, seed 5 with cov3D_precomp
"""
import math

import numpy as np
import torch

from gs4d_train.synthetic import make_camera, make_scene, make_upstream_grad


def _small(seed):
    s = make_scene(60, 70, 45, seed=seed, sh_degree=3, log_scale=math.log(0.08), z_range=(2.0, 6.0))
    s["opacities"] = np.minimum(s["opacities"], 0.9).astype(np.float32)
    return s


def _hi(seed):
    s = _small(seed)
    s["opacities"][::4] = 0.985
    return s


def _rot(seed):
    s = _small(seed)
    cy, sy, cx, sx = math.cos(0.4), math.sin(0.4), math.cos(-0.3), math.sin(-0.3)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R, T = Ry @ Rx, np.array([0.3, -0.2, 0.5])
    cam = make_camera(s["W"], s["H"], R=R, T=T)
    # p_view = R^T p_world + T (the reference's getWorld2View2), so p_world = R (p_view - T)
    s["means3D"] = ((s["means3D"].astype(np.float64) - T) @ R.T).astype(np.float32)
    s["viewmatrix"] = cam.world_view_transform.numpy().astype(np.float32)
    s["projmatrix"] = cam.full_proj_transform.numpy().astype(np.float32)
    s["campos"] = cam.camera_center.numpy().astype(np.float32)
    s["camera"] = cam
    return s


def _dense(seed):
    s = make_scene(300, 40, 24, seed=seed, sh_degree=3, log_scale=math.log(0.25), z_range=(2.0, 6.0))
    s["opacities"] = (0.02 + 0.04 * np.random.default_rng(seed + 50).uniform(0, 1, (300, 1))).astype(np.float32)
    return s


def _cov3d(s):
    from torch_restatement import quat_to_rot
    R = quat_to_rot(torch.tensor(s["rotations"], dtype=torch.float64)).numpy()
    S2 = s["scales"].astype(np.float64) ** 2
    C = np.einsum("pij,pj,pkj->pik", R, S2, R)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1).astype(np.float32)


def _entries():
    out = []
    for kind, make in (("small", _small), ("hi", _hi), ("rot", _rot), ("dense", _dense)):
        for seed in range(4):
            out.append(dict(name=f"{kind}{seed}", make=make, seed=seed, mode="sh"))
    out.append(dict(name="colors4", make=_small, seed=4, mode="colors"))
    out.append(dict(name="cov3D5", make=_small, seed=5, mode="cov3D"))
    return out


ENTRIES = _entries()
NAMES = [e["name"] for e in ENTRIES]
_CACHE = {}


def scene(name):
    """The scene `name`: dict(s=make_scene's dict, colors / cov3D = the precomputed inputs or None, use_sh)."""
    if name not in _CACHE:
        e = ENTRIES[NAMES.index(name)]
        s = e["make"](e["seed"])
        colors = cov3D = None
        if e["mode"] == "colors":
            colors = np.random.default_rng(e["seed"] + 100).uniform(0, 1, (s["means3D"].shape[0], 3)).astype(np.float32)
        if e["mode"] == "cov3D":
            cov3D = _cov3d(s)
        _CACHE[name] = dict(name=name, s=s, colors=colors, cov3D=cov3D, use_sh=e["mode"] != "colors", mode=e["mode"])
    return _CACHE[name]


_REF = {}


def reference(O, name):
    """The oracle's forward of the scene and the fp64 autograd forward over the oracle's sorted lists, made once
    per scene: dict(color, depth, radii, state, export, ref = forward_autograd's dict)."""
    if name not in _REF:
        from gpu_helpers import o_forward
        from torch_restatement import forward_autograd
        sc = scene(name)
        s = sc["s"]
        nr, color, depth, radii, st = o_forward(O, s, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
        ex = st.export()
        # (with cov3D_precomp the restatement builds the same covariance from the scales and rotations)
        ref = forward_autograd(s, ex["point_list"], ex["ranges"], s["sh_degree"],
                               use_precomp_colors=sc["mode"] == "colors", colors=sc["colors"])
        _REF[name] = dict(color=color, depth=depth, radii=radii, state=st, export=ex, ref=ref, nr=nr)
    return _REF[name]


def upstream(name, case):
    """(g_c (3, H, W), g_d (1, H, W)) float32 of a parity case: "depth" g_d ~ N(0, 1) and g_c = 0; "both" the same
    g_d with g_c = make_upstream_grad * 3WH (signs); "sign" g_c = 0 and a +-1 pattern for g_d."""
    sc = scene(name)
    s = sc["s"]
    H, W = s["H"], s["W"]
    seed = ENTRIES[NAMES.index(name)]["seed"]
    rng = np.random.default_rng(1000 + seed)
    g_d = rng.normal(0, 1, (1, H, W)).astype(np.float32)
    g_c = np.zeros((3, H, W), np.float32)
    if case == "both":
        from oracle import oracle as O
        g_c = make_upstream_grad(reference(O, name)["color"], seed=seed + 1)[0] * (3 * W * H)
    elif case == "sign":
        g_d = np.where(rng.uniform(0, 1, (1, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
    else:
        assert case in ("depth", "color")
    if case == "color":  # the colour-only gradient (measures the existing backward's floor F0)
        from oracle import oracle as O
        g_c = make_upstream_grad(reference(O, name)["color"], seed=seed + 1)[0] * (3 * W * H)
        g_d = np.zeros((1, H, W), np.float32)
    return g_c.astype(np.float32), g_d


def autograd_grads(O, name, g_c, g_d):
    """fp64 gradients of sum(color * g_c) + sum(depth * g_d), aligned with _C.rasterize_gaussians_backward's tuple
    (dL_dmeans2D's two columns, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D packed, dL_dsh, dL_dscales,
    dL_drotations); None where the scene's input mode has no such gradient."""
    sc = scene(name)
    ref = reference(O, name)["ref"]
    leaves = [ref["ndc_off"], ref["rgb"], ref["opac"], ref["means"], ref["cov3"], ref["shs"], ref["scales"],
              ref["rots"]]
    loss = (ref["color"] * torch.tensor(g_c, dtype=torch.float64)).sum() + \
        (ref["depth"] * torch.tensor(g_d, dtype=torch.float64)).sum()
    gr = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    z = lambda t, like: np.zeros(tuple(like.shape)) if t is None else t.numpy()
    dm2, dcol, dop, dm3, gc, dsh, dsc, drot = (z(g, l) for g, l in zip(gr, leaves))
    packed = np.stack([gc[:, 0, 0], gc[:, 0, 1] + gc[:, 1, 0], gc[:, 0, 2] + gc[:, 2, 0], gc[:, 1, 1],
                       gc[:, 1, 2] + gc[:, 2, 1], gc[:, 2, 2]], 1)
    return [dm2, dcol, dop, dm3, packed, dsh if sc["mode"] == "sh" else None,
            dsc if sc["mode"] != "cov3D" else None, drot if sc["mode"] != "cov3D" else None]
