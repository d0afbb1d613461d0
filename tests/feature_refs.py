"""References and helpers of the feature-rendering tests (test infrastructure; importable without a GPU).

The feature image of a (P, C) tensor f is F_c(p) = sum_i w_ip f_ic with w = alpha T the forward's blend weights.  Two
references, both trusted elsewhere in this suite:

  A, the composition   for each group of three channels, _C.rasterize_gaussians with colors_precomp = f[:, 3g:3g+3]
                       (zero-padded) over a background of 0 and its backward with dL_dpix = G[3g:3g+3]; the gradients
                       are added over the groups in fp64.  The forward accumulates a colour as C = fma(colour, w, C)
                       in list order and writes C + T_final * 0 = C, so channel c of the feature image must be channel
                       c % 3 of group c // 3 bit for bit.  The geometry does not depend on the colours: every group and
                       the fused pass read the same lists and take the same decisions.
  B, the restatement   torch_restatement.blend's w over the oracle's lists in fp64, (w.unsqueeze(-1) * f[idx]).sum(1),
                       and autograd.  Independent of the GPU; good where no rule of the blend is near its threshold.

The bar of every gradient element is oracle/parity.py's GRAD_RTOL |ref| + GRAD_FLOOR max |ref|.
"""
import math

import numpy as np
import torch

from oracle import parity as PAR

GEOM_NAMES = ["means2D", "opacities", "means3D", "cov3D", "scales", "rotations"]


def features_of(P, C, seed, zero_column=None):
    """(P, C) float32 rows from a seeded normal (both signs); zero_column: that column is all zeros"""
    f = np.random.default_rng(seed).normal(0, 1, (P, C)).astype(np.float32)
    if zero_column is not None and zero_column < C:
        f[:, zero_column] = 0
    return f


def upstream_normal(C, H, W, seed):
    return np.random.default_rng(seed).normal(0, 1, (C, H, W)).astype(np.float32)


def upstream_one_pixel(C, H, W, y, x, channel=None):
    g = np.zeros((C, H, W), np.float32)
    g[C - 1 if channel is None else channel, y, x] = 1.5
    return g


def bar(ref):
    """the parity bar of every element of a gradient with reference `ref` (numpy float64)"""
    ref = np.abs(np.asarray(ref, np.float64))
    return PAR.GRAD_RTOL * ref + PAR.GRAD_FLOOR * (ref.max() if ref.size else 0.0)


def used_of_bar(got, ref):
    """the largest |got - ref| / bar over the elements (0 / 0 counts as 0; x / 0 as inf)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    err, b = np.abs(got - ref), bar(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())


# ---- the GPU side: raw _C calls -------------------------------------------------------------------------------------
def _fwd_args(s, d, colors, cov3D, use_sh):
    e = torch.empty(0, device=d["means3D"].device)
    return (d["bg"], d["means3D"], e if colors is None else colors, d["opacities"],
            e if cov3D is not None else d["scales"], e if cov3D is not None else d["rotations"],
            float(s["scale_modifier"]), e if cov3D is None else cov3D, d["viewmatrix"], d["projmatrix"],
            float(s["tanfovx"]), float(s["tanfovy"]), int(s["H"]), int(s["W"]), d["shs"] if use_sh else e,
            int(s["sh_degree"]), d["campos"], False, False)


def plain_forward(C, s, d, colors=None, cov3D=None, use_sh=True, aa=False):
    args = _fwd_args(s, d, colors, cov3D, use_sh)
    return C.rasterize_gaussians_aa(*args, True) if aa else C.rasterize_gaussians(*args)


def fused_forward(C, s, fwd, feats):
    return C.rasterize_features(feats, fwd[4], fwd[0], fwd[5], fwd[6], feats.shape[0], int(s["H"]), int(s["W"]))


def fused_backward(C, s, d, fwd, feats, grad, cov3D=None, aa=False, geometry=True):
    """(dL_dfeatures, means2D, opacities, means3D, cov3D, scales, rotations) of _C.rasterize_features_backward"""
    e = torch.empty(0, device=d["means3D"].device)
    return C.rasterize_features_backward(
        feats, grad, d["means3D"], fwd[3], e if cov3D is not None else d["scales"],
        e if cov3D is not None else d["rotations"], float(s["scale_modifier"]), e if cov3D is None else cov3D,
        d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), fwd[4], fwd[0], fwd[5], fwd[6],
        d["opacities"] if aa else e, aa, geometry)


def _groups(feats):
    P, Cn = feats.shape
    out = []
    for g in range(0, Cn, 3):
        n = min(3, Cn - g)
        col = torch.zeros(P, 3, device=feats.device)
        col[:, :n] = feats[:, g:g + n]
        out.append((g, n, col))
    return out


def composition_forward(C, s, d, feats, cov3D=None, aa=False):
    """Reference A's image (Cn, H, W) and the forwards of its groups"""
    dz = dict(d)
    dz["bg"] = torch.zeros(3, device=feats.device)
    H, W = int(s["H"]), int(s["W"])
    img = torch.empty(feats.shape[1], H, W, device=feats.device)
    fwds = []
    for g, n, col in _groups(feats):
        fwd = plain_forward(C, s, dz, colors=col, cov3D=cov3D, use_sh=False, aa=aa)
        img[g:g + n] = fwd[1][:n]
        fwds.append((g, n, col, fwd))
    return img, fwds


def composition_backward(C, s, d, feats, grad, cov3D=None, aa=False):
    """Reference A's gradients, float64 numpy: dict(features (P, Cn), means2D, opacities, means3D, cov3D, scales,
    rotations), each the fp64 sum over the groups of three channels"""
    dz = dict(d)
    dz["bg"] = torch.zeros(3, device=feats.device)
    e = torch.empty(0, device=feats.device)
    _, fwds = composition_forward(C, s, d, feats, cov3D=cov3D, aa=aa)
    P, Cn = feats.shape
    out = dict(features=np.zeros((P, Cn)))
    for g, n, col, fwd in fwds:
        gp = torch.zeros(3, int(s["H"]), int(s["W"]), device=feats.device)
        gp[:n] = grad[g:g + n]
        nr, _, _, radii, gb, bb, ib = fwd
        head = (dz["bg"], d["means3D"], radii, col, e if cov3D is not None else d["scales"],
                e if cov3D is not None else d["rotations"], float(s["scale_modifier"]), e if cov3D is None else cov3D,
                d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]))
        tail = (e, int(s["sh_degree"]), d["campos"], gb, nr, bb, ib, False)
        if aa:
            r = C.rasterize_gaussians_backward_aa(*head, gp, e, e, *tail, d["opacities"], True, False)
        else:
            r = C.rasterize_gaussians_backward(*head, gp, *tail)
        m2, dcol, dop, m3, dcov, _, dsc, drot = (t.double().cpu().numpy() for t in r[:8])
        out["features"][:, g:g + n] = dcol[:, :n]
        for k, v in zip(GEOM_NAMES, (m2, dop, m3, dcov, dsc, drot)):
            out[k] = out.get(k, 0) + v
    return out


# ---- Reference B ----------------------------------------------------------------------------------------------------
def restatement(scene, point_list, ranges, cov3D=None):
    """The fp64 graph of the blend weights over the given sorted lists: dict(w (Npix, K), idx (Npix, K), leaves).
    features_image(r, f) then blends a (P, C) float64 tensor; the covariance comes from the scene's scales and
    rotations, or from cov3D (P, 6), whose leaf's gradient is in the packed form."""
    import torch_restatement as TR
    dt = torch.float64
    means = torch.tensor(scene["means3D"], dtype=dt, requires_grad=True)
    scales = torch.tensor(scene["scales"], dtype=dt, requires_grad=True)
    rots = torch.tensor(scene["rotations"], dtype=dt, requires_grad=True)
    opac = torch.tensor(scene["opacities"], dtype=dt, requires_grad=True)
    cov6 = None if cov3D is None else torch.tensor(cov3D, dtype=dt, requires_grad=True)
    W, H = scene["W"], scene["H"]
    cov3 = TR.covariance(scales, rots, float(scene.get("scale_modifier", 1.0)), cov6)
    geo = TR.projected_geometry(scene, means, cov3)
    ndc_off = torch.zeros(means.shape[0], 2, dtype=dt, requires_grad=True)
    pix = ((geo["ndc"] + ndc_off + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
    idx_t, val_t, pxf, pyf = TR.tile_lists(W, H, np.asarray(point_list), np.asarray(ranges))
    bl = TR.blend(pix, geo["conic"], opac, idx_t, val_t, pxf, pyf)
    return dict(w=bl["w"], idx=idx_t, H=H, W=W, means=means, scales=scales, rots=rots, opac=opac, cov6=cov6,
                ndc_off=ndc_off, stats=bl["stats"])


def features_image(r, f):
    """(C, H, W) float64: (w.unsqueeze(-1) * f[idx]).sum(1)"""
    img = (r["w"].unsqueeze(-1) * f[r["idx"]]).sum(1)
    return img.T.reshape(f.shape[1], r["H"], r["W"])


def restatement_grads(r, f, grad):
    """fp64 gradients of sum(F * grad): dict(features, means2D (P, 2), opacities, means3D, cov3D or scales and
    rotations), numpy; f a (P, C) float64 leaf"""
    leaves = dict(features=f, means2D=r["ndc_off"], opacities=r["opac"], means3D=r["means"])
    if r["cov6"] is not None:
        leaves["cov3D"] = r["cov6"]
    else:
        leaves.update(scales=r["scales"], rotations=r["rots"])
    loss = (features_image(r, f) * torch.as_tensor(grad, dtype=torch.float64)).sum()
    gr = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
    return {k: (np.zeros(tuple(l.shape)) if g is None else g.numpy()) for (k, l), g in zip(leaves.items(), gr)}


# ---- the synthetic 4D model of the upper-layer tests ----------------------------------------------------------------
def model_and_views(seed=11, motion=1.0):
    """gs4d_train.synthetic's bouncing_balls (3 x 200 points at t = 0) as a fused GaussianModel whose deformation
    network is re-drawn away from its zero start, so that the timestamps differ; three cameras at two timestamps.
    motion: the weight of the position head's last layer is multiplied by it (the re-drawn network moves a point by about 1e-3
    of the scene's size; the flow tests want pixels)"""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import SH_C0, bouncing_balls, look_at_camera
    hyper, opt = config.dynerf()
    canon, means_at = bouncing_balls(n_per_ball=200, seed=3)
    cols = np.clip(canon["shs"][:, 0, :] * SH_C0 + 0.5, 0, 1).astype(np.float32)
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(means_at(0.0), cols, 1.0)
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
                m.bias.copy_(0.02 * torch.randn_like(m.bias))
        net.pos_deform[3].weight.mul_(motion)  # (not the bias: a shift common to all points is no motion)
    g.training_setup(opt)
    g.active_sh_degree = 3
    cams = [look_at_camera(64, 48, (4.0 * math.sin(0.4 * i), 0.3, -4.0 * math.cos(0.4 * i)), time=(0.0, 0.5, 0.5)[i])
            for i in range(3)]
    return g, cams, hyper, opt
