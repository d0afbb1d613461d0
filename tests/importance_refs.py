"""References and scenes of the blend-weight importance tests (test infrastructure; importable without a GPU).

Two references for gs4d_importance's per-Gaussian scores (the sum and the maximum of w = alpha T over the pixels a
Gaussian blends into, and the number of those pixels):

  reference_scores  the fp64 restatement: torch_restatement.blend's w and contrib over the oracle's sorted lists, an
                    index_add_ for the sum, a scatter_reduce amax for the maximum, the count of contributing slots.
                    Independent of the GPU; good where no rule of the blend is near its threshold.
  onehot_scores     the forward itself: _C.rasterize_gaussians with colors_precomp that is 1 in one channel for each of
                    three chosen Gaussians and 0 elsewhere, over a background of 0.  The blend accumulates
                    C = fma(colour, w, C): fma(1, w, 0) = w and fma(0, w, C) = C exactly, and a pixel takes a given
                    Gaussian at most once, so channel c of the image IS w_ip of that Gaussian, bit for bit, wherever it
                    blends and 0 elsewhere.  The geometry does not depend on the colours, so the lists are the same.
                    Exact everywhere, termination, the cap and the 1/255 rule included.

Scenes: STACK (one tile_list_scenes.stack_scene whose run lengths are the edges of the forward's sort paths and one
run beyond the in-register limit, long enough for its centre pixels to terminate) and WIDE (one large faint Gaussian
over twenty small ones on 256x256 pixels: more than 128 instances of one Gaussian).
"""
import math

import numpy as np
import torch

import tile_list_scenes as TL
from gs4d_train.synthetic import make_scene

STACK_LENGTHS = [0, 1, 2, 64, 65, 128, 129, 256, 257, 513]
STACK_GX = 5
WIDE_BIG = 7  # the large Gaussian's id in the wide scene
_CACHE = {}


def stack_scene():
    """10 tiles (5 x 2) with exactly STACK_LENGTHS Gaussians each, depths with ties"""
    if "stack" not in _CACHE:
        _CACHE["stack"] = TL.stack_scene(STACK_LENGTHS, STACK_GX, 91, "ties")
    return _CACHE["stack"]


def wide_scene():
    """21 Gaussians on 256 x 256 pixels (16 x 16 tiles): twenty small ones and Gaussian WIDE_BIG, isotropic with
    sigma = 70 px and opacity 0.2 behind them all (alpha >= 1/255 within 2.8 sigma: most of the image), so its
    emission slots span more than two waves of the per-Gaussian reduce"""
    if "wide" not in _CACHE:
        s = make_scene(21, 256, 256, seed=23, sh_degree=0, log_scale=math.log(0.04), z_range=(2.0, 4.0), spread=0.8)
        focal_x = s["W"] / (2.0 * s["tanfovx"])
        z = 6.0
        s["means3D"][WIDE_BIG] = [0.05, -0.03, z]
        s["scales"][WIDE_BIG] = 70.0 * z / focal_x
        s["rotations"][WIDE_BIG] = [1, 0, 0, 0]
        s["opacities"][WIDE_BIG] = 0.2
        _CACHE["wide"] = s
    return _CACHE["wide"]


SPARSE_BEHIND, SPARSE_FAINT = [1, 6], [0, 4, 9]


def sparse_culled_scene():
    """alpha_scenes' `sparse` with Gaussians SPARSE_BEHIND moved behind the camera (radii == 0) and SPARSE_FAINT given
    the opacity 0.003 < 1/255 (radii > 0, but no pixel reaches the alpha threshold: the exact culling emits no
    instance of them)"""
    if "sparse_culled" not in _CACHE:
        import alpha_scenes as AS
        s = dict(AS.scene("sparse")["s"])
        s["means3D"] = s["means3D"].copy()
        s["opacities"] = s["opacities"].copy()
        s["means3D"][SPARSE_BEHIND, 2] *= -1
        s["opacities"][SPARSE_FAINT] = 0.003
        _CACHE["sparse_culled"] = s
    return _CACHE["sparse_culled"]


def reference_scores(scene, point_list, ranges):
    """dict(sum (P,) float64, max (P,) float64, count (P,) int64, Tfinal (H, W) float64, stats) from the fp64
    restatement of the blend over the given sorted lists (the oracle's point_list and ranges).  The covariance comes
    from the scene's scales and rotations (a cov3D_precomp scene of depth_scenes is built from them)."""
    import torch_restatement as TR
    dt = torch.float64
    means = torch.tensor(scene["means3D"], dtype=dt)
    cov3 = TR.covariance(torch.tensor(scene["scales"], dtype=dt), torch.tensor(scene["rotations"], dtype=dt),
                         float(scene.get("scale_modifier", 1.0)))
    opac = torch.tensor(scene["opacities"], dtype=dt)
    W, H = scene["W"], scene["H"]
    P = means.shape[0]
    with torch.no_grad():
        geo = TR.projected_geometry(scene, means, cov3)
        pix = ((geo["ndc"] + 1) * torch.tensor([W, H], dtype=dt) - 1) * 0.5
        idx_t, val_t, pxf, pyf = TR.tile_lists(W, H, np.asarray(point_list), np.asarray(ranges))
        bl = TR.blend(pix, geo["conic"], opac, idx_t, val_t, pxf, pyf)
        w = torch.where(bl["contrib"], bl["w"], torch.zeros_like(bl["w"]))
        flat = idx_t.reshape(-1)
        total = torch.zeros(P, dtype=dt).index_add_(0, flat, w.reshape(-1))
        top = torch.zeros(P, dtype=dt).scatter_reduce(0, flat, w.reshape(-1), "amax", include_self=True)
        count = torch.zeros(P, dtype=torch.int64).index_add_(0, flat, bl["contrib"].reshape(-1).to(torch.int64))
    return dict(sum=total, max=top, count=count, Tfinal=bl["Tfinal"].reshape(H, W), stats=bl["stats"])


def onehot_images(C, s, d, ids, cov3D=None, antialiasing=False):
    """(3, H, W) float32 device tensor: channel c is the blend weight of Gaussian ids[c] at every pixel (0 where it
    does not blend).  d = gpu_helpers.to_dev(s, device); fewer than three ids leave the last channels 0."""
    dev = d["means3D"].device
    P = d["means3D"].shape[0]
    colors = torch.zeros(P, 3, device=dev)
    for c, i in enumerate(ids):
        colors[int(i), c] = 1.0
    e = torch.empty(0, device=dev)
    args = (torch.zeros(3, device=dev), d["means3D"], colors, d["opacities"], e if cov3D is not None else d["scales"],
            e if cov3D is not None else d["rotations"], float(s["scale_modifier"]), e if cov3D is None else cov3D,
            d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), int(s["H"]), int(s["W"]), e,
            int(s["sh_degree"]), d["campos"], False, False)
    out = C.rasterize_gaussians_aa(*args, True) if antialiasing else C.rasterize_gaussians(*args)
    return out[1]


def onehot_scores(C, s, d, ids, cov3D=None, antialiasing=False):
    """For each Gaussian of `ids`, three per forward: dict(ids, max (n,) float32 = the one-hot image's maximum,
    count (n,) int64 = its non-zero pixels, sum (n,) float64 = the fp64 sum of its pixels), on the host."""
    ids = [int(i) for i in ids]
    mx, cnt, tot = [], [], []
    for k in range(0, len(ids), 3):
        chunk = ids[k:k + 3]
        img = onehot_images(C, s, d, chunk, cov3D=cov3D, antialiasing=antialiasing)
        flat = img.reshape(3, -1)[:len(chunk)]
        mx.append(flat.max(1).values.cpu())
        cnt.append((flat != 0).sum(1).cpu())
        tot.append(flat.double().sum(1).cpu())
    if not ids:
        return dict(ids=ids, max=torch.zeros(0), count=torch.zeros(0, dtype=torch.int64),
                    sum=torch.zeros(0, dtype=torch.float64))
    return dict(ids=ids, max=torch.cat(mx), count=torch.cat(cnt), sum=torch.cat(tot))


def sum_bound(count, total):
    """count * 2^-24 * total: the bound on |fl(sum) - sum| for ANY order of adding `count` non-negative floats whose
    exact sum is `total` (see tests/test_importance_gpu.py's docstring)"""
    return count.double() * 2.0 ** -24 * total
