"""Independent float64 autograd restatement of the rasterizer forward (test infrastructure).

Used to cross-check the C oracle's hand-derived backward (backward.cu restated) against automatic
differentiation of the forward math (forward.cu restated in plain matrix form, NOT the glm
column-major transcription), on small scenes.  Per-pixel blending is vectorised over padded per-tile
lists taken from the oracle's sort.

The reference's non-differentiable rules (SURVEY §8 a) are restated the way its own backward treats them, so
autograd of this forward is the reference's gradient wherever no decision sits on its threshold (the returned
margins say how far each one is):

  Q22  the frustum clamp of computeCov2D: where |t.x / t.z| > 1.3 tan_fov, J[0][2] takes the clamped t.x as a
       CONSTANT (dL_dtx = 0 and dL_dtz keeps its clamped-t.x term, backward.cu:262-264) -- not torch.clamp's
       autograd, which would differentiate clamp(t.x / t.z) * t.z through t.z as well
  Q26  the covariance is built from scale_modifier * scales and dL_dscales is NOT multiplied by the modifier
       (backward.cu:278-341): the reference's value is this restatement's autograd gradient / scale_modifier
  Q17  alpha = min(0.99, o G) in the value with a straight-through gradient (backward.cu:486-503 recomputes the
       capped alpha and differentiates o G)
  power > 0 is skipped (forward.cu:341-342; only a conic that is not positive definite, from cov3D_precomp, gets
       there), alpha < 1/255 is skipped, and a pixel retires at the first contributing slot whose T (1 - alpha)
       < 1e-4: that slot and every later one do not blend (forward.cu:349-354)

The scenes of tests/depth_scenes.py keep every one of these inactive; tests/rule_scenes.py holds the scenes on
which they bind.
"""
import math

import numpy as np
import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]
ALPHA_MIN = 1.0 / 255.0
ALPHA_CAP = 0.99
T_MIN = 1e-4
CLAMP_FACTOR = 1.3


def eval_sh_torch(deg, sh, d):
    """sh (P,K,3), d (P,3) unit -> (P,3); same polynomial as forward.cu:20-62."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    r = SH_C0 * sh[:, 0]
    if deg > 0:
        r = r - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * sh[:, 6]
             + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        r = (r + SH_C3[0] * y * (3 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
             + SH_C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
             + SH_C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
             + SH_C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return r


def quat_to_rot(q):
    """Standard rotation matrix of an (r,x,y,z) quaternion used as-is (no normalisation, forward.cu:127)."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    return R


def covariance(scales, rots, scale_modifier=1.0, cov6=None):
    """(P, 3, 3) world covariance: R diag((scale_modifier * scales)^2) R^T, or the symmetric matrix of the packed
    cov3D_precomp rows [00, 01, 02, 11, 12, 22] (any symmetric matrix, positive definite or not)."""
    if cov6 is not None:
        c = cov6
        return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]],
                           1).reshape(-1, 3, 3)
    s = scale_modifier * scales
    R = quat_to_rot(rots)
    return R @ torch.diag_embed(s * s) @ R.transpose(1, 2)


def projected_geometry(scene, means, cov3):
    """The per-Gaussian geometry of preprocessCUDA in float64 (forward.cu:74-113, 189-240), differentiable in
    `means` and `cov3`: dict(ndc (P, 2) before any screen-space offset, t (P, 3) view coordinates, conic (P, 3),
    clamped (P, 2) bool = the Q22 clamp binds in x / y, clamp_dist (P, 2) = ||t.x / t.z| - lim| / lim)."""
    dt = means.dtype
    V = torch.tensor(scene["viewmatrix"], dtype=dt).reshape(4, 4)   # flat column-major -> p_h @ V
    Pm = torch.tensor(scene["projmatrix"], dtype=dt).reshape(4, 4)
    W, H = scene["W"], scene["H"]
    tfx, tfy = scene["tanfovx"], scene["tanfovy"]
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    P = means.shape[0]
    ph = torch.cat([means, torch.ones(P, 1, dtype=dt)], 1)
    phom = ph @ Pm
    pw = 1.0 / (phom[:, 3:4] + 1e-7)
    ndc = phom[:, :2] * pw
    t = (ph @ V)[:, :3]
    Rv = V[:3, :3].T                                                     # rotation part of the view transform
    tz = t[:, 2]
    lim = torch.tensor([CLAMP_FACTOR * tfx, CLAMP_FACTOR * tfy], dtype=dt)
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
    a = cov2[:, 0, 0] + 0.3
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    return dict(ndc=ndc, t=t, conic=conic, clamped=clamped, clamp_dist=clamp_dist)


def tile_lists(W, H, point_list, ranges):
    """The oracle's sorted per-tile lists, padded to the longest and gathered per pixel: idx (Npix, K) Gaussian ids,
    val (Npix, K) slot validity, px / py (Npix, 1) pixel coordinates (float64)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (ys // 16) * gx + (xs // 16)
    lens = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    K = max(int(lens.max()) if lens.size else 0, 1)
    idx = np.zeros((gx * gy, K), np.int64)
    valid = np.zeros((gx * gy, K), bool)
    for ti in range(gx * gy):
        s, e = int(ranges[ti, 0]), int(ranges[ti, 1])
        idx[ti, :e - s] = point_list[s:e]
        valid[ti, :e - s] = True
    idx_t = torch.from_numpy(idx)[tile.reshape(-1)]          # (Npix, K)
    val_t = torch.from_numpy(valid)[tile.reshape(-1)]
    return idx_t, val_t, xs.reshape(-1, 1).to(torch.float64), ys.reshape(-1, 1).to(torch.float64)


def blend(pix, conic, opac, idx_t, val_t, pxf, pyf):
    """renderCUDA's walk (forward.cu:330-366) over the padded lists.  pix: the splat centres in pixels, (P, 2) or per
    slot (Npix, K, 2); conic (P, 3); opac (P, 1).  Returns dict(w (Npix, K) blend weights alpha T, Tfinal (Npix,),
    contrib (Npix, K) bool = the slot blends, and the plain-number margins of forward_autograd's dict)."""
    dt = conic.dtype
    if pix.dim() == 2:
        pix = pix[idx_t]
    dx = pix[..., 0] - pxf
    dy = pix[..., 1] - pyf
    co = conic[idx_t]
    power = -0.5 * (co[..., 0] * dx * dx + co[..., 2] * dy * dy) - co[..., 1] * dx * dy
    keep = power <= 0                                                    # forward.cu:341-342
    # the exponent is masked BEFORE exp: an overflowing exp under a where() turns the gradients to NaN
    raw = opac[idx_t, 0] * torch.exp(torch.where(keep, power, torch.zeros_like(power)))
    alpha = raw + (torch.clamp_max(raw, ALPHA_CAP) - raw).detach()       # Q17: capped value, straight-through gradient
    contrib = val_t & keep & (alpha >= ALPHA_MIN)
    K = idx_t.shape[1]
    with torch.no_grad():
        # T (1 - alpha) of every contributing slot as long as the pixel has not retired; the first one below
        # 1e-4 retires it (that slot and every later one do not blend)
        a0 = torch.where(contrib, alpha, torch.zeros_like(alpha))
        test_T = torch.cumprod(1 - a0, 1)
        hit = contrib & (test_T < T_MIN)
        pos = torch.arange(K).unsqueeze(0)
        first = torch.where(hit, pos, torch.full_like(pos, K)).min(1, keepdim=True).values
        alive = pos < first
        walked = contrib & (pos <= first)                                # blended slots and the terminating one
        term_dist = torch.where(walked, (test_T / T_MIN - 1).abs(), torch.full_like(test_T, math.inf))
    contrib = contrib & alive
    a_m = torch.where(contrib, alpha, torch.zeros_like(alpha))
    Tcum = torch.cumprod(torch.cat([torch.ones(a_m.shape[0], 1, dtype=dt), 1 - a_m], 1), 1)
    Tbefore, Tfinal = Tcum[:, :-1], Tcum[:, -1]
    w = a_m * Tbefore
    # the margins and counts the callers compare with the oracle or assert on the scene
    with torch.no_grad():
        nonpd = ~((conic[:, 0] > 0) & (conic[:, 0] * conic[:, 2] - conic[:, 1] ** 2 > 0))
        # pairs of a splat with a conic that is not positive definite whose o exp(power) reaches 1/255: the sign of
        # the power decides them, in units of the magnitude of the power's terms
        big = val_t & nonpd[idx_t] & (torch.log(opac[idx_t, 0].clamp_min(1e-300)) + power >= math.log(ALPHA_MIN))
        mag = 0.5 * co[..., 0].abs() * dx * dx + 0.5 * co[..., 2].abs() * dy * dy + (co[..., 1] * dx * dy).abs()
        pdist = torch.where(big, power.abs() / mag.clamp_min(1e-300), torch.full_like(power, math.inf))
        near = val_t & keep & ((raw - ALPHA_MIN).abs() < 1e-8)
        ncontrib = torch.where(contrib, pos + 1, torch.zeros_like(pos)).max(1).values
        stats = dict(
            n_contrib=ncontrib.numpy(), near_threshold=int(near.sum()),
            clamp099=int((val_t & keep & (raw > ALPHA_CAP)).sum()),      # valid pairs above the cap, blended or not
            cap_blended=int((contrib & (raw > ALPHA_CAP)).sum()),        # ... of them, the ones that blend
            min_T=float(Tfinal.min()), n_terminated=int((first < K).sum()), term_margin=float(term_dist.min()),
            n_power_rejected=int((val_t & ~keep).sum()), power_margin=float(pdist.min()),
            nonpd=nonpd.numpy(),
            nonpd_contributes=np.bincount(idx_t[contrib & nonpd[idx_t]].numpy(), minlength=conic.shape[0]) > 0)
    return dict(w=w, Tfinal=Tfinal, contrib=contrib, stats=stats)


def forward_autograd(scene, point_list, ranges, degree, use_precomp_colors=False, colors=None, cov3D=None):
    """Differentiable float64 forward.  Returns dict of outputs and leaf tensors.

    scene: numpy arrays (means3D, scales, rotations, opacities, shs, bg, viewmatrix, projmatrix,
    campos, tanfovx, tanfovy, W, H) and optionally scale_modifier.  point_list/ranges: the oracle's sorted per-tile
    lists.  cov3D: (P, 6) cov3D_precomp rows; they become the leaf `cov6`, whose gradient is already in the
    reference's packed form [00, 01+10, 02+20, 11, 12+21, 22], and scales / rotations are not used.

    Next to the outputs: n_contrib (H, W), near_threshold, clamp099 (valid pairs whose o G exceeds the cap),
    cap_blended (those of them that blend), min_T, and the margins of the rules in the module docstring:
    n_clamped / clamped (P,) / clamp_margin over the Gaussians in the lists, n_terminated pixels and term_margin
    = min |T (1 - alpha) / 1e-4 - 1| over blended and terminating slots, n_power_rejected pairs and power_margin
    = min |power| / (1/2 |a| dx^2 + 1/2 |c| dy^2 + |b dx dy|) over the pairs of a non-positive-definite conic with
    o exp(power) >= 1/255, nonpd (P,) and nonpd_contributes (P,)."""
    dt = torch.float64
    means = torch.tensor(scene["means3D"], dtype=dt, requires_grad=True)
    scales = torch.tensor(scene["scales"], dtype=dt, requires_grad=True)
    rots = torch.tensor(scene["rotations"], dtype=dt, requires_grad=True)
    opac = torch.tensor(scene["opacities"], dtype=dt, requires_grad=True)
    shs = torch.tensor(scene["shs"], dtype=dt, requires_grad=True)
    cov6 = None if cov3D is None else torch.tensor(cov3D, dtype=dt, requires_grad=True)
    campos = torch.tensor(scene["campos"], dtype=dt)
    W, H = scene["W"], scene["H"]
    mod = float(scene.get("scale_modifier", 1.0))
    P = means.shape[0]

    cov3 = covariance(scales, rots, mod, cov6)
    cov3.retain_grad()
    geo = projected_geometry(scene, means, cov3)
    t = geo["t"]
    ndc_off = torch.zeros(P, 2, dtype=dt, requires_grad=True)          # screenspace_points trick
    ndc = geo["ndc"] + ndc_off
    pix = ((ndc + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5

    if use_precomp_colors:
        rgb = torch.tensor(colors, dtype=dt, requires_grad=True)
        rgb_leaf = rgb
    else:
        d = means - campos
        d = d / d.norm(dim=1, keepdim=True)
        rgb = torch.clamp_min(eval_sh_torch(degree, shs, d) + 0.5, 0.0)
        rgb_leaf = None
    rgb.retain_grad() if rgb_leaf is None else None

    idx_t, val_t, pxf, pyf = tile_lists(W, H, point_list, ranges)
    bl = blend(pix, geo["conic"], opac, idx_t, val_t, pxf, pyf)
    w, Tfinal, st = bl["w"], bl["Tfinal"], bl["stats"]
    col = (w.unsqueeze(-1) * rgb[idx_t]).sum(1) + Tfinal.unsqueeze(-1) * torch.tensor(scene["bg"], dtype=dt)
    depth = (w * t[idx_t, 2]).sum(1)
    # the clamp's margins, over the Gaussians the lists hold
    listed = np.zeros(P, bool)
    listed[np.asarray(point_list, np.int64)] = True
    clamped = geo["clamped"].any(1).numpy() & listed
    dist = geo["clamp_dist"].min(1).values.numpy()
    out = dict(color=col.T.reshape(3, H, W), depth=depth.reshape(1, H, W), Tfinal=Tfinal.reshape(H, W),
               means=means, scales=scales, rots=rots, opac=opac, shs=shs, ndc_off=ndc_off, rgb=rgb, cov3=cov3,
               cov6=cov6, scale_modifier=mod, clamped=clamped, n_clamped=int(clamped.sum()),
               clamp_margin=float(dist[listed].min()) if listed.any() else math.inf)
    out.update(st)
    out["n_contrib"] = st["n_contrib"].reshape(H, W)
    return out
