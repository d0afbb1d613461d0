"""fp64 reference of the camera gradient (test infrastructure): tests/torch_restatement.py's graph with the view
matrix V, the full projection Pm and the camera centre c as leaves, and the scenes it is compared on.

torch_restatement.forward_autograd holds the three as constants.  Here `projected_geometry` and the direction line
are restated with them as tensors (same arithmetic: the clamp still holds the clamped t.x / t.y as a constant, Q22),
and covariance / blend / tile_lists / eval_sh_torch are torch_restatement's own.  `antialiasing` multiplies the
opacity by tests/antialias_refs.py's factor s, restated on the same covariance.

The camera enters in four linear steps: t = ([m, 1] V)[:3] (the depth included), Rv = V[:3, :3]^T in Tm = J Rv,
p_hom = [m, 1] Pm and dir = m - c.  camera_reference() returns autograd's 35 gradients of the leaves, and from
autograd's gradients of the four steps' results each Gaussian's term of each family, hence the four families' sums
and the mass A[k] = sum_i |term_i[k]| with term_i the sum of Gaussian i's families at element k.

The scenes keep tests/rule_scenes.py's size (P <= 300, at most 70 x 45):
  cam_sh       depth_scenes' small scene, SH degree 3, seen by a rotated, translated camera
  cam_colors   rule_scenes' clamp scene with colors_precomp (rotated camera, focal_x != focal_y)
  cam_clamp    rule_scenes' clamp1: a quarter of the visible Gaussians beyond the frustum clamp
  cam_dense    depth_scenes' dense scene (P = 300, 40 x 24, every splat over most of the six tiles, about 1500
               instances): Gaussians whose records straddle two waves of the reduction, so their sums are finished
               inside the per-Gaussian kernel.  No splat can have more than 15 instances at this image size (15
               tiles); what the kernel does differently is decided by the straddling, which the GPU test asserts
  cam_behind   cam_sh's recipe with every third Gaussian behind the near plane (view z <= 0.2: culled, radii 0)
"""
import math

import numpy as np
import torch

import depth_scenes as DS
import rule_scenes as RS
import torch_restatement as TR

AA_FLOOR = 2.5e-5
LOW_PASS = 0.3
FAMILIES = ("t", "W", "proj", "campos")


def projected_geometry(scene, means, cov3, V, Pm, antialiasing=False):
    """torch_restatement.projected_geometry, line for line, with V and Pm (4, 4) given as tensors; adds phom, Tm, J
    (whose gradients give the per-Gaussian terms) and s (P,), the antialiasing factor (ones without it)."""
    dt = means.dtype
    W, H = scene["W"], scene["H"]
    tfx, tfy = scene["tanfovx"], scene["tanfovy"]
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    P = means.shape[0]
    ph = torch.cat([means, torch.ones(P, 1, dtype=dt)], 1)
    phom = ph @ Pm
    pw = 1.0 / (phom[:, 3:4] + 1e-7)
    ndc = phom[:, :2] * pw
    t = (ph @ V)[:, :3]
    Rv = V[:3, :3].T
    tz = t[:, 2]
    lim = torch.tensor([TR.CLAMP_FACTOR * tfx, TR.CLAMP_FACTOR * tfy], dtype=dt)
    with torch.no_grad():
        ratio = t[:, :2] / tz.unsqueeze(1)
        clamped = ratio.abs() > lim
        held = torch.maximum(torch.minimum(ratio, lim), -lim) * tz.unsqueeze(1)   # a constant of the backward
        clamp_dist = (ratio.abs() - lim).abs() / lim
    txy = torch.where(clamped, held, t[:, :2])
    J = torch.zeros(P, 3, 3, dtype=dt)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * txy[:, 0] / tz ** 2
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * txy[:, 1] / tz ** 2
    Tm = J @ Rv
    cov2 = Tm @ cov3 @ Tm.transpose(1, 2)
    a0, b0, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    a = cov2[:, 0, 0] + 0.3
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    s = torch.ones_like(det)
    if antialiasing:
        r = (a0 * c0 - b0 * b0) / det
        floored = (r <= AA_FLOOR).detach()
        s = torch.sqrt(torch.where(floored, torch.full_like(r, AA_FLOOR), r))
    return dict(ndc=ndc, t=t, conic=conic, clamped=clamped, clamp_dist=clamp_dist, s=s, ph=ph, phom=phom, Tm=Tm, J=J)


def forward_autograd(scene, point_list, ranges, degree, use_precomp_colors=False, colors=None, cov3D=None,
                     antialiasing=False, camera_leaves=True):
    """torch_restatement.forward_autograd's dict with V (4, 4), Pm (4, 4), c (3,) as fp64 leaves (camera_leaves=False:
    constants, the graph then being forward_autograd's own), and the intermediates t, phom, Tm, dirs that each use of
    the camera produces, kept for camera_reference."""
    dt = torch.float64
    means = torch.tensor(scene["means3D"], dtype=dt, requires_grad=True)
    scales = torch.tensor(scene["scales"], dtype=dt, requires_grad=True)
    rots = torch.tensor(scene["rotations"], dtype=dt, requires_grad=True)
    opac = torch.tensor(scene["opacities"], dtype=dt, requires_grad=True)
    shs = torch.tensor(scene["shs"], dtype=dt, requires_grad=True)
    cov6 = None if cov3D is None else torch.tensor(cov3D, dtype=dt, requires_grad=True)
    V = torch.tensor(scene["viewmatrix"], dtype=dt).reshape(4, 4).requires_grad_(camera_leaves)
    Pm = torch.tensor(scene["projmatrix"], dtype=dt).reshape(4, 4).requires_grad_(camera_leaves)
    campos = torch.tensor(scene["campos"], dtype=dt).requires_grad_(camera_leaves)
    W, H = scene["W"], scene["H"]
    mod = float(scene.get("scale_modifier", 1.0))
    P = means.shape[0]

    cov3 = TR.covariance(scales, rots, mod, cov6)
    cov3.retain_grad()
    geo = projected_geometry(scene, means, cov3, V, Pm, antialiasing)
    t = geo["t"]
    ndc_off = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    ndc = geo["ndc"] + ndc_off
    pix = ((ndc + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
    dirs = None
    if use_precomp_colors:
        rgb = torch.tensor(colors, dtype=dt, requires_grad=True)
    else:
        dirs = means - campos
        d = dirs / dirs.norm(dim=1, keepdim=True)
        rgb = torch.clamp_min(TR.eval_sh_torch(degree, shs, d) + 0.5, 0.0)
        rgb.retain_grad()
    opac_eff = opac * geo["s"].unsqueeze(1) if antialiasing else opac
    idx_t, val_t, pxf, pyf = TR.tile_lists(W, H, point_list, ranges)
    bl = TR.blend(pix, geo["conic"], opac_eff, idx_t, val_t, pxf, pyf)
    w, Tfinal, st = bl["w"], bl["Tfinal"], bl["stats"]
    col = (w.unsqueeze(-1) * rgb[idx_t]).sum(1) + Tfinal.unsqueeze(-1) * torch.tensor(scene["bg"], dtype=dt)
    depth = (w * t[idx_t, 2]).sum(1)
    listed = np.zeros(P, bool)
    listed[np.asarray(point_list, np.int64)] = True
    clamped = geo["clamped"].any(1).numpy() & listed
    dist = geo["clamp_dist"].min(1).values.numpy()
    out = dict(color=col.T.reshape(3, H, W), depth=depth.reshape(1, H, W), Tfinal=Tfinal.reshape(H, W),
               means=means, scales=scales, rots=rots, opac=opac, shs=shs, ndc_off=ndc_off, rgb=rgb, cov3=cov3,
               cov6=cov6, scale_modifier=mod, clamped=clamped, n_clamped=int(clamped.sum()),
               clamp_margin=float(dist[listed].min()) if listed.any() else math.inf, listed=listed,
               V=V, Pm=Pm, c=campos, t=t, ph=geo["ph"], phom=geo["phom"], Tm=geo["Tm"], J=geo["J"], dirs=dirs)
    out.update(st)
    out["n_contrib"] = st["n_contrib"].reshape(H, W)
    return out


def loss_of(ref, g_c, g_d, g_a):
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return (ref["color"] * f64(g_c)).sum() + (ref["depth"] * f64(g_d)).sum() + \
        ((1.0 - ref["Tfinal"]) * f64(g_a).reshape(ref["Tfinal"].shape)).sum()


def camera_reference(ref, g_c, g_d, g_a):
    """dict(grad (35,) = autograd's dL/dV, dL/dPm, dL/dc flattened; families = {name: (35,)} the four families' sums;
    A (35,) the mass; dV, dPm, dc; dmeans (P, 3), dcov (P, 3, 3) = dL/dmeans3D and dL/dcov3D of the same loss).
    A Gaussian's term of a family is the product rule of the one linear step that uses the camera, from autograd's
    gradient of that step's result: t = [m, 1] V gives p_h (x) dL/dt, p_hom = [m, 1] Pm gives p_h (x) dL/dp_hom,
    Tm = J Rv gives (J^T dL/dTm)^T and dir = m - c gives -dL/ddir; their sums are checked against autograd's leaves."""
    loss = loss_of(ref, g_c, g_d, g_a)
    wanted = [ref["V"], ref["Pm"], ref["c"], ref["means"], ref["cov3"], ref["t"], ref["phom"], ref["Tm"]]
    if ref["dirs"] is not None:
        wanted.append(ref["dirs"])
    gr = torch.autograd.grad(loss, wanted, retain_graph=True, allow_unused=True)
    z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()
    dV, dPm, dc, dmeans, dcov, dt_, dphom, dTm = (z(g, l) for g, l in zip(gr[:8], wanted[:8]))
    ddir = z(gr[8], wanted[8]) if len(gr) > 8 else np.zeros_like(dmeans)
    P = dmeans.shape[0]
    ph, J = ref["ph"].detach().numpy(), ref["J"].detach().numpy()
    z16, z3 = np.zeros((P, 16)), np.zeros((P, 3))
    t_term = np.zeros((P, 4, 4))
    t_term[:, :, :3] = ph[:, :, None] * dt_[:, None, :]
    w_term = np.zeros((P, 4, 4))
    w_term[:, :3, :3] = np.einsum("pab,pak->pkb", J, dTm)          # dL/dRv = J^T dL/dTm, transposed into V's layout
    terms = dict(t=np.concatenate([t_term.reshape(P, 16), z16, z3], 1),
                 W=np.concatenate([w_term.reshape(P, 16), z16, z3], 1),
                 proj=np.concatenate([z16, (ph[:, :, None] * dphom[:, None, :]).reshape(P, 16), z3], 1),
                 campos=np.concatenate([z16, z16, -ddir], 1))
    total = sum(terms.values())
    grad = np.concatenate([dV.reshape(-1), dPm.reshape(-1), dc.reshape(-1)])
    assert np.allclose(total.sum(0), grad, rtol=1e-9, atol=1e-11 * max(1.0, np.abs(grad).max()))
    return dict(grad=grad, families={k: v.sum(0) for k, v in terms.items()}, A=np.abs(total).sum(0), dV=dV, dPm=dPm,
                dc=dc, dmeans=dmeans, dcov=dcov)


def bar(A):
    """the parity bar of every element: GRAD_RTOL A[k] + GRAD_FLOOR max_k A[k] (oracle/parity.py's constants)"""
    from oracle import parity as PAR
    return PAR.GRAD_RTOL * A + PAR.GRAD_FLOOR * A.max()


def translation_residual(V, Pm, dV, dPm, dc, dmeans):
    """both sides of the translation identity, (3,) each: moving the camera rigidly by -d is moving every mean by d"""
    lhs = dV[3, :] @ V.T[:, :3] + dPm[3, :] @ Pm.T[:, :3] - dc
    return lhs, dmeans.sum(0)


# ---- scenes ----------------------------------------------------------------------------------------------------
def _rotated(s):
    """depth_scenes._rot's camera applied to a scene given in view coordinates"""
    cy, sy, cx, sx = math.cos(0.4), math.sin(0.4), math.cos(-0.3), math.sin(-0.3)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R, T = Ry @ Rx, np.array([0.3, -0.2, 0.5])
    from gs4d_train.synthetic import make_camera
    cam = make_camera(s["W"], s["H"], R=R, T=T)
    s["means3D"] = ((s["means3D"].astype(np.float64) - T) @ R.T).astype(np.float32)
    s["viewmatrix"] = cam.world_view_transform.numpy().astype(np.float32)
    s["projmatrix"] = cam.full_proj_transform.numpy().astype(np.float32)
    s["campos"] = cam.camera_center.numpy().astype(np.float32)
    s["camera"] = cam
    return s


def _behind(seed):
    s = DS._small(seed)
    P = s["means3D"].shape[0]
    z = np.random.default_rng(seed + 70).uniform(-3.0, 0.15, P).astype(np.float32)
    s["means3D"][::3, 2] = z[::3]          # view z <= 0.2: behind the near plane
    return _rotated(s)


BEHIND_SEED = 0
ENTRIES = [
    dict(name="cam_sh", make=lambda seed: DS._rot(seed), seed=1, mode="sh"),
    dict(name="cam_colors", make=RS._clamp, seed=4, mode="colors"),
    dict(name="cam_clamp", make=RS._clamp, seed=1, mode="sh"),
    dict(name="cam_dense", make=DS._dense, seed=1, mode="sh"),
    dict(name="cam_behind", make=_behind, seed=BEHIND_SEED, mode="sh"),
]
NAMES = [e["name"] for e in ENTRIES]
COLOR_NAMES = [e["name"] for e in ENTRIES if e["mode"] == "colors"]
_CACHE, _REF, _CAMREF = {}, {}, {}


def build(e):
    s = e["make"](e["seed"])
    colors = None
    if e["mode"] == "colors":
        colors = np.random.default_rng(e["seed"] + 100).uniform(0, 1, (s["means3D"].shape[0], 3)).astype(np.float32)
    return dict(name=e["name"], s=s, colors=colors, cov3D=None, use_sh=colors is None, mode=e["mode"], seed=e["seed"])


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = build(ENTRIES[NAMES.index(name)])
    return _CACHE[name]


def make_reference(O, sc, antialiasing=False, fold=None):
    """the oracle's forward (its sorted lists) and the fp64 graph with camera leaves over them.  antialiasing: the
    lists are those of the folded plain problem, opacities fl32(o s) with s from fp64 (tests/antialias_scenes.py's
    construction), since the factor moves neither radii nor rectangles."""
    from gpu_helpers import o_forward
    s = sc["s"] if fold is None else fold
    nr, color, depth, radii, st = o_forward(O, s, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    ex = st.export()
    ref = forward_autograd(sc["s"], ex["point_list"], ex["ranges"], sc["s"]["sh_degree"],
                           use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"],
                           antialiasing=antialiasing)
    return dict(color=color, depth=depth, radii=radii, state=st, export=ex, ref=ref, nr=nr, scene=s)


def reference(O, name, antialiasing=False):
    key = (name, bool(antialiasing))
    if key not in _REF:
        sc = scene(name)
        fold = None
        if antialiasing:
            import antialias_refs as AAR
            s64 = AAR.factor(sc["s"], sc["cov3D"])[0]
            fold = dict(sc["s"])
            fold["opacities"] = (sc["s"]["opacities"].astype(np.float64) * s64[:, None]).astype(np.float32)
        _REF[key] = make_reference(O, sc, antialiasing, fold)
    return _REF[key]


def upstream(O, name, case):
    """rule_scenes.upstream's three images for the scene: "color", "both" (+ depth), "all" (+ alpha)"""
    from gs4d_train.synthetic import make_upstream_grad
    assert case in ("color", "both", "all")
    sc = scene(name)
    s, seed = sc["s"], sc["seed"]
    H, W = s["H"], s["W"]
    g_d = np.random.default_rng(1000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_a = np.random.default_rng(2000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_c = (make_upstream_grad(reference(O, name)["color"], seed=seed + 1)[0] * (3 * W * H)).astype(np.float32)
    if case == "color":
        g_d = np.zeros_like(g_d)
    if case != "all":
        g_a = np.zeros_like(g_a)
    return g_c, g_d, g_a


def camera_ref(O, name, case, antialiasing=False):
    """camera_reference of the scene under upstream(case), made once"""
    key = (name, case, bool(antialiasing))
    if key not in _CAMREF:
        _CAMREF[key] = camera_reference(reference(O, name, antialiasing)["ref"], *upstream(O, name, case))
    return _CAMREF[key]


# ---- the reduction's edges: a 32 x 32 image, unit upstream gradients -------------------------------------------
# the per-Gaussian kernels' workgroups are 256 threads with colors_precomp and 128 with SHs: the last Gaussian at
# the end of a wave or workgroup and one to either side, and 700 for three rows and more
EDGE_P = [1, 127, 128, 129, 255, 256, 257, 700]


def edge_scene(P, mode):
    from gs4d_train.synthetic import make_scene
    seed = 40 + P
    s = make_scene(P, 32, 32, seed=seed, sh_degree=3, log_scale=math.log(0.06), z_range=(2.0, 6.0))
    s["opacities"] = (0.02 + 0.1 * s["opacities"]).astype(np.float32)       # faint: no cap, no termination
    colors = None
    if mode == "colors":
        colors = np.random.default_rng(P).uniform(0, 1, (P, 3)).astype(np.float32)
    return dict(name=f"edge{P}{mode}", s=s, colors=colors, cov3D=None, use_sh=colors is None, mode=mode, seed=seed)
