"""fp64 restatement of the antialiased rasterizer forward (test infrastructure).

tests/torch_restatement.py's forward with the opacity compensated for the 0.3 px^2 low-pass (Mip-Splatting's 2-D
filter, include/gs4d.h gs4d_forward_aa).  With (a0, b, c0) the projected covariance before the low-pass,
a = a0 + 0.3, c = c0 + 0.3:

    D0 = a0 c0 - b^2    D1 = a c - b^2    r = D0 / D1    s = sqrt(max(2.5e-5, r))    o_eff = o s

The floor is a constant of the backward: where r <= 2.5e-5, s is the number 0.005 and no gradient reaches the
covariance through it (torch.where on a detached mask).  The conic, and so the lists, are those of the dilated
covariance; `o s` goes to torch_restatement.blend in place of `o`.  torch_restatement is imported unchanged.
"""
import math

import numpy as np
import torch

import torch_restatement as TR

AA_FLOOR = 2.5e-5
LOW_PASS = 0.3


def projected_geometry(scene, means, cov3):
    """torch_restatement.projected_geometry's dict (same arithmetic, restated here because the covariance before
    the low-pass is needed) plus r, s (P,), floored (P,) bool and kappa (P,) = (a0 c0 + b^2) / |D0|, the condition
    number of D0 with respect to relative errors of its two products."""
    dt = means.dtype
    V = torch.tensor(scene["viewmatrix"], dtype=dt).reshape(4, 4)
    Pm = torch.tensor(scene["projmatrix"], dtype=dt).reshape(4, 4)
    W, H = scene["W"], scene["H"]
    tfx, tfy = scene["tanfovx"], scene["tanfovy"]
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    P = means.shape[0]
    ph = torch.cat([means, torch.ones(P, 1, dtype=dt)], 1)
    phom = ph @ Pm
    ndc = phom[:, :2] * (1.0 / (phom[:, 3:4] + 1e-7))
    t = (ph @ V)[:, :3]
    Rv = V[:3, :3].T
    tz = t[:, 2]
    lim = torch.tensor([TR.CLAMP_FACTOR * tfx, TR.CLAMP_FACTOR * tfy], dtype=dt)
    with torch.no_grad():
        ratio = t[:, :2] / tz.unsqueeze(1)
        clamped = ratio.abs() > lim
        held = torch.maximum(torch.minimum(ratio, lim), -lim) * tz.unsqueeze(1)   # Q22: a constant of the backward
        clamp_dist = (ratio.abs() - lim).abs() / lim
    txy = torch.where(clamped, held, t[:, :2])
    J = torch.zeros(P, 3, 3, dtype=dt)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * txy[:, 0] / tz ** 2
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * txy[:, 1] / tz ** 2
    Tm = J @ Rv
    cov2 = Tm @ cov3 @ Tm.transpose(1, 2)
    a0, b, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    a, c = a0 + LOW_PASS, c0 + LOW_PASS
    D0 = a0 * c0 - b * b
    D1 = a * c - b * b
    conic = torch.stack([c / D1, -b / D1, a / D1], 1)
    r = D0 / D1
    floored = (r <= AA_FLOOR).detach()
    # sqrt is taken of a value that stays away from 0 on both branches: a where() over sqrt(r) alone would turn
    # the gradient of a floored Gaussian with r <= 0 into NaN
    s = torch.sqrt(torch.where(floored, torch.full_like(r, AA_FLOOR), r))
    with torch.no_grad():
        kappa = (a0 * c0 + b * b) / D0.abs().clamp_min(1e-300)
    return dict(ndc=ndc, t=t, conic=conic, clamped=clamped, clamp_dist=clamp_dist, r=r, s=s,
                floored=floored, kappa=kappa)


def factor(scene, cov3D=None):
    """(s, r, floored, kappa) of the scene as float64 / bool numpy arrays (P,), no gradients"""
    dt = torch.float64
    with torch.no_grad():
        cov3 = TR.covariance(torch.tensor(scene["scales"], dtype=dt), torch.tensor(scene["rotations"], dtype=dt),
                             float(scene.get("scale_modifier", 1.0)),
                             None if cov3D is None else torch.tensor(cov3D, dtype=dt))
        geo = projected_geometry(scene, torch.tensor(scene["means3D"], dtype=dt), cov3)
    return geo["s"].numpy(), geo["r"].numpy(), geo["floored"].numpy(), geo["kappa"].numpy()


def forward_autograd(scene, point_list, ranges, degree, use_precomp_colors=False, colors=None, cov3D=None):
    """torch_restatement.forward_autograd with the compensated opacity: colour, depth and Tfinal built the same way
    from blend(pix, conic, opac * s, ...); the leaves are the same, `opac` the RAW opacity.  Adds s, r, floored,
    kappa (numpy, (P,)) and opac_eff (P, 1) to its dict."""
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

    cov3 = TR.covariance(scales, rots, mod, cov6)
    cov3.retain_grad()
    geo = projected_geometry(scene, means, cov3)
    t = geo["t"]
    ndc_off = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    pix = ((geo["ndc"] + ndc_off + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
    if use_precomp_colors:
        rgb = torch.tensor(colors, dtype=dt, requires_grad=True)
    else:
        d = means - campos
        rgb = torch.clamp_min(TR.eval_sh_torch(degree, shs, d / d.norm(dim=1, keepdim=True)) + 0.5, 0.0)
        rgb.retain_grad()
    opac_eff = opac * geo["s"].unsqueeze(1)
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
               s=geo["s"].detach().numpy(), r=geo["r"].detach().numpy(), floored=geo["floored"].numpy(),
               kappa=geo["kappa"].numpy(), opac_eff=opac_eff, conic=geo["conic"],
               blends=np.bincount(idx_t[bl["contrib"]].numpy(), minlength=P) > 0)
    out.update(st)
    out["n_contrib"] = st["n_contrib"].reshape(H, W)
    return out
