"""Instant4D grid pruning of the initial point cloud (the reference's `use_grid_pruning` switch).

What the reference does with utils/grid_pruning.py and the block scene/__init__.py:102-127 that calls it: the
initial cloud is replaced by one averaged point per occupied voxel before `create_from_pcd`.  The reference hands
the voxel grid to Open3D on the host; here it is gs4d_voxel_downsample (csrc/voxel.hip) on the device, with a
defined row order.  The voxel sizes are host numpy, restated operation for operation so they come out bitwise as
the reference's.  Normals are not carried: `create_from_pcd` never reads them.

`GaussianModel`, `create_from_pcd`, `render()` and `train_step()` do not know about this module; a caller opts in
through `initialize(..., use_grid_pruning=True)`.

The other end of training is here too (no reference counterpart): `prune_by_importance` removes the Gaussians of a
trained or training model that deposit little in any of a set of (camera, time) views, by the blend-weight scores
of `infer.importance` -- RadSplat's rule on the largest weight, LightGaussian's / Mini-Splatting's ranking by the
summed weight or the hit count.  The training loop calls it where it wants; `train_step()` does not.
"""
import math

import numpy as np
import torch

__all__ = ["voxel_downsample", "adaptive_voxel_size", "grid_pruning", "grid_pruning_with_motion", "initialize"]
# (importance_mask and prune_by_importance, the score-based pruning, are reached by name: the star import stays the
# grid pruning's surface)


def _device_f32(x, device="cuda"):
    if torch.is_tensor(x):
        return (x if x.is_cuda else x.to(device)).float()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(device)


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def voxel_downsample(points, colors, voxel_size):
    """utils/grid_pruning.py:16-41 on the device: (points (M, 3), colors (M, 3) or None) as device tensors, one row
    per occupied voxel of size `voxel_size`, rows ascending in the voxels' linear index.  Arrays and CPU tensors
    are copied to the current device; `colors` may be None."""
    from . import _C
    pts = _device_f32(points)
    cols = None if colors is None else _device_f32(colors, pts.device)
    p, c, _ = _C.voxel_downsample(pts, cols, float(voxel_size))
    return p, c


def _focal_pair(cam):
    """(width, height, FovX, FovY) of the reference's CameraInfo (FovX / FovY) or of gs4d_train.camera.Camera
    (FoVx / FoVy, image_width / image_height)."""
    fovx = cam.FovX if hasattr(cam, "FovX") else cam.FoVx
    fovy = cam.FovY if hasattr(cam, "FovY") else cam.FoVy
    width = cam.width if hasattr(cam, "width") else cam.image_width
    height = cam.height if hasattr(cam, "height") else cam.image_height
    return width, height, fovx, fovy


def adaptive_voxel_size(points, cameras=None, focal_mean=None, depth_mean=None, scale_factor=3.0):
    """utils/grid_pruning.py:44-96: voxel = mean depth / mean focal * scale_factor, clamped to [0.001, 1].  The
    depth of a camera is the median distance of the points from its centre, its focal length the mean of fx and
    fy from the fields of view; without cameras, the median distance from the centroid and a focal of 1000."""
    points = _host(points)
    if cameras is not None and len(cameras) > 0:
        depths = []
        focals = []
        for cam in cameras:
            cam_center = -np.matmul(cam.R.T, cam.T)
            dists = np.linalg.norm(points - cam_center.reshape(1, 3), axis=1)
            depths.append(np.median(dists))
            width, height, fovx, fovy = _focal_pair(cam)
            fx = width / (2 * np.tan(fovx / 2))
            fy = height / (2 * np.tan(fovy / 2))
            focals.append((fx + fy) / 2)
        depth_mean = np.mean(depths) if depth_mean is None else depth_mean
        focal_mean = np.mean(focals) if focal_mean is None else focal_mean
    if depth_mean is None:
        depth_mean = np.percentile(np.linalg.norm(points - points.mean(axis=0), axis=1), 50)
    if focal_mean is None:
        focal_mean = 1000.0
    voxel_size = depth_mean / focal_mean * scale_factor
    voxel_size = max(voxel_size, 0.001)
    voxel_size = min(voxel_size, 1.0)
    return voxel_size


def grid_pruning(points, colors, cameras=None, use_adaptive=True, static_scale=4.0, dynamic_scale=3.0):
    """utils/grid_pruning.py:99-161: with cameras (an empty list included, as in the reference) the adaptive size
    at the mean of the two scales, otherwise the bounding box's diagonal / 100; then the device downsample.
    Returns (points, colors) on the device."""
    host = _host(points)
    if use_adaptive and cameras is not None:
        avg_scale = (static_scale + dynamic_scale) / 2
        voxel_size = adaptive_voxel_size(host, cameras, scale_factor=avg_scale)
    else:
        bbox_diagonal = np.linalg.norm(host.max(axis=0) - host.min(axis=0))
        voxel_size = bbox_diagonal / 100.0
    return voxel_downsample(points, colors, voxel_size)


def grid_pruning_with_motion(points, colors, motion_prob=None, cameras=None, static_scale=4.0, dynamic_scale=3.0,
                             threshold=0.7):
    """utils/grid_pruning.py:164-265: points with motion_prob > threshold are dynamic.  The static part is pruned
    at the static scale's voxel size, then the dynamic part at the dynamic scale's, and the rows are concatenated
    in that order.  Returns (points, colors, motion) with motion the 0 / 1 flag per row (float64, as the
    reference's); without motion_prob, the single-size path and motion = None."""
    if motion_prob is None:
        avg_scale = (static_scale + dynamic_scale) / 2
        voxel_size = adaptive_voxel_size(points, cameras, scale_factor=avg_scale)
        p, c = voxel_downsample(points, colors, voxel_size)
        return p, c, None
    host_p, host_c = _host(points), _host(colors)
    dynamic_mask = _host(motion_prob) > threshold
    static_mask = ~dynamic_mask
    out_p, out_c, out_m = [], [], []
    for mask, scale, flag in ((static_mask, static_scale, 0.0), (dynamic_mask, dynamic_scale, 1.0)):
        if mask.sum() > 0:
            part_p, part_c = host_p[mask], host_c[mask]
            voxel_size = adaptive_voxel_size(part_p, cameras, scale_factor=scale)
            p, c = voxel_downsample(part_p, part_c, voxel_size)
            out_p.append(p)
            out_c.append(c)
            out_m.append(torch.full((p.shape[0],), flag, dtype=torch.float64, device=p.device))
    if not out_p:  # an empty cloud (the reference's np.vstack of nothing raises)
        raise ValueError("grid_pruning_with_motion: no points")
    return torch.cat(out_p), torch.cat(out_c), torch.cat(out_m)


def initialize(gaussians, points, colors, spatial_lr_scale, cameras=None, use_grid_pruning=False):
    """scene/__init__.py:85-127 for a fresh model: the field's bounds from the UNPRUNED cloud's max / min (:85-91),
    the cloud pruned with the first ten cameras when asked (:106-119), then create_from_pcd (:127).  With
    use_grid_pruning=False this is set_aabb followed by create_from_pcd on the cloud as given."""
    host = _host(points)
    xyz_max = host.max(axis=0)
    xyz_min = host.min(axis=0)
    gaussians._deformation.deformation_net.grid.set_aabb(xyz_max.tolist(), xyz_min.tolist())
    if use_grid_pruning:
        try:
            train_cams = cameras[:10] if hasattr(cameras, "__getitem__") else []
        except Exception:
            train_cams = None
        p, c = grid_pruning(points, colors, cameras=train_cams, use_adaptive=True, static_scale=4.0, dynamic_scale=3.0)
        # create_from_pcd takes host arrays (it is not touched): the pruned cloud makes one round trip
        points, colors = p.cpu().numpy(), c.cpu().numpy()
    gaussians.create_from_pcd(points, colors, spatial_lr_scale)


def importance_mask(scores, min_max_weight=None, keep_fraction=None, by="sum"):
    """The boolean prune mask (True = remove) from `infer.importance`'s scores.  A row is pruned if
    scores["max"] < min_max_weight (RadSplat's rule), and also if it falls outside the top ceil(keep_fraction * P)
    rows by scores[by] ("sum", "max", "count" or "views"), ties going to the lower index; both conditions are OR-ed.
    ValueError when neither is given, for keep_fraction outside (0, 1] and for an unknown `by`."""
    if min_max_weight is None and keep_fraction is None:
        raise ValueError("importance_mask: give min_max_weight, keep_fraction or both")
    if by not in ("sum", "max", "count", "views") or by not in scores:
        raise ValueError(f"importance_mask: unknown score {by!r}")
    if keep_fraction is not None and not (0.0 < keep_fraction <= 1.0):
        raise ValueError("importance_mask: keep_fraction must lie in (0, 1]")
    P = scores["max"].shape[0]
    prune = torch.zeros(P, dtype=torch.bool, device=scores["max"].device)
    if min_max_weight is not None:
        prune |= scores["max"] < min_max_weight
    if keep_fraction is not None:
        keep = min(P, math.ceil(keep_fraction * P))
        order = torch.sort(scores[by], descending=True, stable=True).indices  # equal scores: the lower index first
        outside = torch.ones(P, dtype=torch.bool, device=prune.device)
        outside[order[:keep]] = False
        prune |= outside
    return prune


def prune_by_importance(gaussians, cameras, min_max_weight=None, keep_fraction=None, by="sum", antialiasing=False):
    """Score `gaussians` over `cameras` and remove the rows importance_mask selects: infer.prepare, infer.importance,
    importance_mask, then gaussians.prune_points(mask), i.e. the fused row surgery, so the optimizer state and the
    densification statistics stay consistent.  Returns (n_removed, scores), the scores being those of the model
    before the removal.  Call it where the schedule wants it (after the last densification, before an export);
    an InferenceState prepared earlier is stale afterwards."""
    from . import infer
    importance_mask({"max": torch.zeros(0), by: torch.zeros(0)}, min_max_weight, keep_fraction, by)  # argument errors first
    state = infer.prepare(gaussians)
    scores = infer.importance(state, cameras, antialiasing=antialiasing)
    mask = importance_mask(scores, min_max_weight, keep_fraction, by)
    n_removed = int(mask.sum())
    if n_removed:
        gaussians.prune_points(mask)
    return n_removed, scores
