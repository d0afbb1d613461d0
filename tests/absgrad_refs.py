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

from torch_restatement import blend, covariance, eval_sh_torch, projected_geometry, tile_lists


def per_pixel_forward(scene, point_list, ranges, degree, colors=None, cov3D=None):
    """color (3, H, W), depth (1, H, W) in fp64 and the per-(pixel, slot) leaf `pix_off` (Npix, K, 2), with
    idx (Npix, K) Gaussian ids and val (Npix, K) slot validity.  The forward's math is forward_autograd's (the same
    functions: projected_geometry, tile_lists, blend, so every rule restated there holds here); only the leaf
    differs, so nothing but `pix_off` requires a gradient."""
    dt = torch.float64
    t64 = lambda k: torch.tensor(scene[k], dtype=dt)
    means, scales, rots, opac, shs = t64("means3D"), t64("scales"), t64("rotations"), t64("opacities"), t64("shs")
    campos = t64("campos")
    W, H = scene["W"], scene["H"]
    P = means.shape[0]
    cov3 = covariance(scales, rots, float(scene.get("scale_modifier", 1.0)),
                      None if cov3D is None else torch.tensor(cov3D, dtype=dt))
    geo = projected_geometry(scene, means, cov3)
    ndc, t = geo["ndc"], geo["t"]
    if colors is not None:
        rgb = torch.tensor(colors, dtype=dt)
    else:
        d = means - campos
        rgb = torch.clamp_min(eval_sh_torch(degree, shs, d / d.norm(dim=1, keepdim=True)) + 0.5, 0.0)

    idx_t, val_t, pxf, pyf = tile_lists(W, H, point_list, ranges)
    pix_off = torch.zeros(H * W, idx_t.shape[1], 2, dtype=dt, requires_grad=True)   # the one leaf
    pix = ((ndc[idx_t] + pix_off + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
    bl = blend(pix, geo["conic"], opac, idx_t, val_t, pxf, pyf)
    w = bl["w"]
    col = (w.unsqueeze(-1) * rgb[idx_t]).sum(1) + bl["Tfinal"].unsqueeze(-1) * torch.tensor(scene["bg"], dtype=dt)
    depth = (w * t[idx_t, 2]).sum(1)
    return dict(color=col.T.reshape(3, H, W), depth=depth.reshape(1, H, W), Tfinal=bl["Tfinal"].reshape(H, W),
                pix_off=pix_off, idx=idx_t, val=val_t, P=P)


def absgrad_reference(fw, g_c, g_d=None, signed_want=None, g_a=None):
    """(absgrad (P, 2), signed (P, 2)) in fp64 for the upstream gradients g_c (3, H, W), g_d (1, H, W) or None and
    g_a (1, H, W) or None (of the alpha image 1 - Tfinal).
    signed_want: the existing restatement's ndc_off gradient (P, 2); when given, the signed scatter-sum must equal it
    to 1e-12 of its largest element."""
    loss = (fw["color"] * torch.tensor(np.asarray(g_c), dtype=torch.float64)).sum()
    if g_d is not None:
        loss = loss + (fw["depth"] * torch.tensor(np.asarray(g_d), dtype=torch.float64)).sum()
    if g_a is not None:
        loss = loss + ((1.0 - fw["Tfinal"]) * torch.tensor(np.asarray(g_a), dtype=torch.float64)[0]).sum()
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
