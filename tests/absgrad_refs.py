"""fp64 reference of the absolute screen-space gradient (absgrad) over the oracle's sorted lists (test
infrastructure).

The dense restatement of tests/torch_restatement.forward_autograd with one more leaf: an NDC offset per (pixel,
list slot), shape (Npix, K, 2), added where `ndc_off` is added.  autograd.grad of sum(color * g_c) + sum(depth * g_d)
with respect to that leaf is every pixel's own term of `means2D.grad` (in its units: the NDC offset reaches the pixel
coordinate through the same W / 2, H / 2); absgrad is the sum over a Gaussian's valid slots of its absolute value,
and the signed sum must be the existing restatement's `ndc_off` gradient (checked here, 1e-12 relative).
"""
import numpy as np
import torch

from torch_restatement import eval_sh_torch, quat_to_rot


def per_pixel_forward(scene, point_list, ranges, degree, colors=None):
    """color (3, H, W), depth (1, H, W) in fp64 and the per-(pixel, slot) leaf `pix_off` (Npix, K, 2), with
    idx (Npix, K) Gaussian ids and val (Npix, K) slot validity.  The forward's math is forward_autograd's; only the
    leaf differs, so nothing but `pix_off` requires a gradient."""
    dt = torch.float64
    t64 = lambda k: torch.tensor(scene[k], dtype=dt)
    means, scales, rots, opac, shs = t64("means3D"), t64("scales"), t64("rotations"), t64("opacities"), t64("shs")
    V, Pm, campos = t64("viewmatrix").reshape(4, 4), t64("projmatrix").reshape(4, 4), t64("campos")
    W, H = scene["W"], scene["H"]
    fx, fy = W / (2 * scene["tanfovx"]), H / (2 * scene["tanfovy"])
    P = means.shape[0]
    ph = torch.cat([means, torch.ones(P, 1, dtype=dt)], 1)
    phom = ph @ Pm
    ndc = phom[:, :2] / (phom[:, 3:4] + 1e-7)
    t = (ph @ V)[:, :3]
    R = quat_to_rot(rots)
    cov3 = R @ torch.diag_embed(scales * scales) @ R.transpose(1, 2)
    tz = t[:, 2]
    J = torch.zeros(P, 3, 3, dtype=dt)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * t[:, 0] / tz ** 2
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * t[:, 1] / tz ** 2
    Tm = J @ V[:3, :3].T
    cov2 = Tm @ cov3 @ Tm.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    if colors is not None:
        rgb = torch.tensor(colors, dtype=dt)
    else:
        d = means - campos
        rgb = torch.clamp_min(eval_sh_torch(degree, shs, d / d.norm(dim=1, keepdim=True)) + 0.5, 0.0)

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
    idx_t = torch.from_numpy(idx)[tile.reshape(-1)]
    val_t = torch.from_numpy(valid)[tile.reshape(-1)]
    pix_off = torch.zeros(H * W, K, 2, dtype=dt, requires_grad=True)   # the one leaf
    pix = ((ndc[idx_t] + pix_off + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
    dx = pix[..., 0] - xs.reshape(-1, 1).to(dt)
    dy = pix[..., 1] - ys.reshape(-1, 1).to(dt)
    co = conic[idx_t]
    power = -0.5 * (co[..., 0] * dx * dx + co[..., 2] * dy * dy) - co[..., 1] * dx * dy
    alpha = opac[idx_t, 0] * torch.exp(power)
    contrib = val_t & (power <= 0) & (alpha >= 1.0 / 255.0) & (alpha <= 0.99)
    a_m = torch.where(contrib, alpha, torch.zeros_like(alpha))
    Tcum = torch.cumprod(torch.cat([torch.ones(a_m.shape[0], 1, dtype=dt), 1 - a_m], 1), 1)
    w = a_m * Tcum[:, :-1]
    col = (w.unsqueeze(-1) * rgb[idx_t]).sum(1) + Tcum[:, -1:] * torch.tensor(scene["bg"], dtype=dt)
    depth = (w * t[idx_t, 2]).sum(1)
    return dict(color=col.T.reshape(3, H, W), depth=depth.reshape(1, H, W), pix_off=pix_off, idx=idx_t, val=val_t, P=P)


def absgrad_reference(fw, g_c, g_d=None, signed_want=None):
    """(absgrad (P, 2), signed (P, 2)) in fp64 for the upstream gradients g_c (3, H, W) and g_d (1, H, W) or None.
    signed_want: the existing restatement's ndc_off gradient (P, 2); when given, the signed scatter-sum must equal it
    to 1e-12 of its largest element."""
    loss = (fw["color"] * torch.tensor(np.asarray(g_c), dtype=torch.float64)).sum()
    if g_d is not None:
        loss = loss + (fw["depth"] * torch.tensor(np.asarray(g_d), dtype=torch.float64)).sum()
    (g,) = torch.autograd.grad(loss, [fw["pix_off"]], retain_graph=True)
    g = torch.where(fw["val"].unsqueeze(-1), g, torch.zeros_like(g)).reshape(-1, 2)
    ids = fw["idx"].reshape(-1)
    absg = torch.zeros(fw["P"], 2, dtype=torch.float64).index_add_(0, ids, g.abs())
    signed = torch.zeros(fw["P"], 2, dtype=torch.float64).index_add_(0, ids, g)
    if signed_want is not None:
        want = np.asarray(signed_want, np.float64)[:, :2]
        err = float(np.abs(signed.numpy() - want).max())
        assert err <= 1e-12 * max(float(np.abs(want).max()), 1e-300), f"signed scatter-sum off by {err:.3e}"
    return absg.numpy(), signed.numpy()


_FW = {}


def scene_forward(O, name):
    """per_pixel_forward of the tests/depth_scenes.py scene `name`, over the oracle's lists, made once"""
    if name not in _FW:
        import depth_scenes as DS
        sc, ref = DS.scene(name), DS.reference(O, name)
        s = sc["s"]
        _FW[name] = per_pixel_forward(s, ref["export"]["point_list"], ref["export"]["ranges"], s["sh_degree"],
                                      colors=sc["colors"] if sc["mode"] == "colors" else None)
    return _FW[name]


def scene_absgrad(O, name, g_c, g_d):
    """the reference absgrad of a depth_scenes scene for (g_c, g_d), the sanity check against
    depth_scenes.autograd_grads' dL_dmeans2D included"""
    import depth_scenes as DS
    want = DS.autograd_grads(O, name, g_c, g_d)[0]
    return absgrad_reference(scene_forward(O, name), g_c, g_d, signed_want=want)[0]
