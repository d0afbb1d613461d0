"""The inference path: a trained model played back, evaluated or exported, one frame per timestamp.

What the reference does with render.py (render_set and its FPS figure, :57-70), metrics.py (per-image PSNR / SSIM
means), export_perframe_3DGS.py (:55-73, :100-106) and utils/render_utils.get_state_at_time (:3-18).  At inference
the planes, the MLP's weights and the canonical means are constants and only the time changes, so `prepare`
captures them once -- the planes packed channels-last, the Morton order of the canonical means, the active heads'
first layers stacked -- and a frame's deformation is three launches: the field's points (gs4d_hexplane_points), the
field over the packed planes (gs4d_hexplane_forward) and gs4d_deform_infer (csrc/deform_infer.hip), which takes the
field features to the rasterizer's five inputs without writing h, a or the deltas.

A configuration outside that kernel's shapes (state.fused False: another width, defor_depth > 1, CPU tensors, ...)
runs the torch formulation of render() under no_grad instead, with its results.  gs4d_train.render.render is
untouched; this module is what a caller opts into.
"""
import copy
import math
import time as _time

import torch

from .render import _time_float, _time_value

__all__ = ["prepare", "state_at_time", "get_state_at_time", "render_view", "render_set", "evaluate"]
# (infer.importance, the opt-in blend-weight scores, is reached by name: the star import stays the playback surface)

# (head, the flag that switches it off, GS4D_ROLE_* of include/gs4d_train.h), in forward_dynamic's order
_HEADS = (("pos_deform", "no_dx", 0), ("scales_deform", "no_ds", 1), ("rotations_deform", "no_dr", 2),
          ("opacity_deform", "no_do", 3), ("shs_deform", "no_dshs", 4))
_SHAPES = ((32, 128), (48, 128), (64, 64), (32, 64))  # (feat_dim, W) gs4d_deform_infer is built for (_FeatureReLU.shapes)


class InferenceState:
    """What prepare() captured.  The bases (xyz, scaling, rotation, opacity, f_dc, f_rest) are references to the
    model's tensors as they were; the planes and the MLP's weights are copies.  fused: the HIP path serves it."""

    def __init__(self):
        self.fused = False
        self.stage = "fine"
        self.active_sh_degree = 0
        self.xyz = self.scaling = self.rotation = self.opacity = self.f_dc = self.f_rest = None
        self.zero_points = None   # the rasterizer's means2D, a zero (P, 3) buffer
        self.deformation = None   # fallback: a copy of the deformation network
        # fused: the field (packed planes, their sizes, the point order) and the MLP
        self.aabb = self.packed = self.order = None
        self.plane_f, self.plane_w, self.plane_h = 0, [], []
        self.wf = self.bf = self.w1 = self.b1 = None
        self.w2, self.b2, self.roles = [], [], []


def _active(args):
    return [(name, role) for name, flag, role in _HEADS if not getattr(args, flag)]


@torch.no_grad()
def prepare(gaussians, stage="fine"):
    """Capture `gaussians` for inference at `stage` ("fine": deformed by the field; "coarse": the canonical
    Gaussians, tail only).  A capture, not a view: after an optimizer step, densify, prune or load, prepare again
    (a stale state keeps reading the old model's memory, which it holds on to)."""
    if "coarse" not in stage and "fine" not in stage:
        raise NotImplementedError(stage)
    pc = gaussians
    st = InferenceState()
    st.stage = "coarse" if "coarse" in stage else "fine"
    st.active_sh_degree = pc.active_sh_degree
    st.xyz, st.scaling, st.rotation, st.opacity, st.f_dc, st.f_rest = (
        t.detach() for t in (pc.get_xyz, pc._scaling, pc._rotation, pc._opacity, pc._features_dc, pc._features_rest))
    st.zero_points = torch.zeros_like(st.xyz)
    bases = (st.xyz, st.scaling, st.rotation, st.opacity, st.f_dc, st.f_rest)
    on_gpu = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in bases)
    if st.stage == "coarse":
        st.fused = on_gpu
        return st
    net = pc._deformation.deformation_net
    a = net.args
    active = _active(a)
    lin = net.feature_out[0]
    K = st.f_rest.shape[1] + 1
    st.fused = bool(
        on_gpu and active and len(net.feature_out) == 1 and (lin.in_features, net.W) in _SHAPES
        and not a.apply_rotation and (K == 16 or all(name != "shs_deform" for name, _ in active))
        and st.xyz.shape[1] == 3 and st.xyz.shape[0] > 0
        and all(p.is_cuda and p.dtype == torch.float32 for p in net.parameters()))
    if not st.fused:
        st.deformation = copy.deepcopy(pc._deformation).requires_grad_(False)
        return st
    from . import _C
    planes = [p.detach() for level in net.grid.grids for p in level]
    st.aabb = net.grid.aabb.detach().clone()
    st.plane_f = planes[0].shape[1]
    st.plane_w, st.plane_h = [p.shape[3] for p in planes], [p.shape[2] for p in planes]
    # one evaluation of the field (at t = 0) packs the planes channels-last and orders the points: the Morton order
    # is of x, y, z alone, so it serves every timestamp
    t0 = _time_value(0.0, st.xyz.device).expand(st.xyz.shape[0], 1)
    _, st.packed, st.order = _C.hexplane_forward(_C.hexplane_points(st.xyz, t0, st.aabb), planes, None)
    heads = [getattr(net, name) for name, _ in active]
    st.wf, st.bf = lin.weight.detach().clone(), lin.bias.detach().clone()
    st.w1 = torch.cat([hd[1].weight.detach() for hd in heads], 0).contiguous()
    st.b1 = torch.cat([hd[1].bias.detach() for hd in heads], 0).contiguous()
    st.w2 = [hd[3].weight.detach().clone() for hd in heads]
    st.b2 = [hd[3].bias.detach().clone() for hd in heads]
    st.roles = [role for _, role in active]
    return st


def _torch_state(state, t, activate):
    """render()'s torch formulation under no_grad (gaussian_renderer/__init__.py:79-99)."""
    import torch.nn.functional as F
    xyz = state.xyz
    shs = torch.cat((state.f_dc, state.f_rest), dim=1)
    if state.stage == "coarse":
        m3, sc, rot, op, sh = xyz, state.scaling, state.rotation, state.opacity, shs
    else:
        time = _time_value(t, xyz.device).expand(xyz.shape[0], 1)
        m3, sc, rot, op, sh = state.deformation(xyz, state.scaling, state.rotation, state.opacity, shs, time)
    if activate:
        sc, rot, op = torch.exp(sc), F.normalize(rot), torch.sigmoid(op)
    return m3, sc, rot, op, sh


@torch.no_grad()
def state_at_time(state, t, activate=True):
    """(means3D, scales, rotations, opacity, shs) of the Gaussians at time t: the rasterizer's inputs with
    activate=True, the deformed raw parameters (a PLY's columns) with activate=False."""
    t = _time_float(t)
    if not state.fused:
        return _torch_state(state, t, activate)
    from . import _C
    xyz = state.xyz
    if state.stage == "coarse":
        if not activate:
            return _torch_state(state, t, False)
        return tuple(_C.deform_tail_forward(xyz, state.scaling, state.rotation, state.opacity, state.f_dc, state.f_rest,
                                            None, None, None, None, None))
    time = _time_value(t, xyz.device).expand(xyz.shape[0], 1)
    pts = _C.hexplane_points(xyz, time, state.aabb)
    feat = _C.hexplane_forward_packed(pts, state.packed, state.plane_f, state.plane_w, state.plane_h, state.order)
    try:
        return tuple(_C.deform_infer(feat, state.wf, state.bf, state.w1, state.b1, state.w2, state.b2, state.roles, xyz,
                                     state.scaling, state.rotation, state.opacity, state.f_dc, state.f_rest, activate))
    except RuntimeError as e:
        if "status 4" in str(e):  # GS4D_TRAIN_ERR_LDS: no quiet fall-back, the caller has gs4d_train.render.render
            raise RuntimeError("gs4d_deform_infer: this device cannot give the kernel its LDS; use "
                               "gs4d_train.render.render for this model") from e
        raise


def get_state_at_time(state, camera):
    """utils/render_utils.py:3-18, its quirk included: the deformed, un-activated means, scales and rotations, the
    UNDEFORMED opacity parameter, and the deformed SHs, at the camera's time."""
    m3, sc, rot, _, sh = state_at_time(state, camera.time, activate=False)
    return m3, sc, rot, state.opacity, sh


def _raster_settings(camera, state, bg, scaling_modifier=1.0, camera_tensors=None):
    """render()'s GaussianRasterizationSettings for `camera` (gaussian_renderer/__init__.py:37-55)."""
    import diff_gaussian_rasterization as dgr
    dev = state.xyz.device
    if camera_tensors is not None:
        view_m, proj_m, cam_c = (t.detach() for t in camera_tensors)
    elif hasattr(camera, "on_device"):
        view_m, proj_m, cam_c = camera.on_device(dev)
    else:
        view_m, proj_m, cam_c = (camera.world_view_transform.to(dev), camera.full_proj_transform.to(dev),
                                 camera.camera_center.to(dev))
    return dgr.GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width),
        tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5), bg=bg,
        scale_modifier=scaling_modifier, viewmatrix=view_m, projmatrix=proj_m, sh_degree=state.active_sh_degree,
        campos=cam_c, prefiltered=False, debug=False)


@torch.no_grad()
def render_view(camera, state, bg, scaling_modifier=1.0, antialiasing=False, camera_tensors=None, features=None):
    """render()'s dict (gaussian_renderer/__init__.py:130-138) for a captured model, through the same rasterizer.
    antialiasing: render()'s switch; a model trained with it on is rendered with it on.  camera_tensors: render()'s
    (viewmatrix, projmatrix, campos) in place of the camera's own, e.g. a refined pose (PoseRefiner.tensors).
    features: render()'s (P, C) rows, or a callable of the deformed means; the dict gains "features" (C, H, W), the
    forward pass only."""
    import diff_gaussian_rasterization as dgr
    settings = _raster_settings(camera, state, bg, scaling_modifier, camera_tensors)
    m3, sc, rot, op, sh = state_at_time(state, camera.time, activate=True)
    extra = {}
    if features is not None:
        extra["features"] = features(m3) if callable(features) else features
    out = dgr.GaussianRasterizer(raster_settings=settings, antialiasing=antialiasing)(
        means3D=m3, means2D=state.zero_points, shs=sh, colors_precomp=None, opacities=op, scales=sc, rotations=rot,
        cov3D_precomp=None, **extra)
    image, radii, depth = out[:3]
    pkg = {"render": image, "viewspace_points": state.zero_points, "visibility_filter": radii > 0, "radii": radii,
           "depth": depth}
    if features is not None:
        pkg["features"] = out[3]
    return pkg


@torch.no_grad()
def importance(state, cameras, antialiasing=False):
    """Blend-weight importance of every Gaussian over `cameras` ((camera, time) views): {"sum", "max", "count",
    "views"}, four (P,) tensors.  For each camera, in order: the state at its time, one forward, and the pass that
    keeps what the forward's blend deposited (diff_gaussian_rasterization.gaussian_importance).  With w = alpha * T
    of a (pixel, Gaussian) pair: "sum" (float64) adds each view's per-Gaussian sum of w, view by view in list order
    (LightGaussian's / Mini-Splatting's importance); "max" (float32) is the largest w over all rays (RadSplat's
    score); "count" (int64) the number of pixels reached (LightGaussian's hit count); "views" (int64) the number
    of views with radii > 0.  The same camera list gives the same bits."""
    import diff_gaussian_rasterization as dgr
    dev = state.xyz.device
    P = state.xyz.shape[0]
    out = {"sum": torch.zeros(P, dtype=torch.float64, device=dev), "max": torch.zeros(P, dtype=torch.float32, device=dev),
           "count": torch.zeros(P, dtype=torch.int64, device=dev), "views": torch.zeros(P, dtype=torch.int64, device=dev)}
    bg = torch.zeros(3, dtype=torch.float32, device=dev)  # the weights do not depend on it
    for cam in cameras:
        settings = _raster_settings(cam, state, bg)
        m3, sc, rot, op, sh = state_at_time(state, cam.time, activate=True)
        wsum, wmax, count, radii = dgr.gaussian_importance(m3, op, shs=sh, scales=sc, rotations=rot,
                                                           raster_settings=settings, antialiasing=antialiasing)
        out["sum"] += wsum.double()
        out["max"] = torch.maximum(out["max"], wmax)
        out["count"] += count.long()
        out["views"] += (radii > 0).long()
    return out


def _sync(state):
    if state.xyz.is_cuda:
        torch.cuda.synchronize(state.xyz.device)


def render_set(state, cameras, bg, keep_images=True, antialiasing=False):
    """(images, fps): every camera rendered in order, and the reference's frame rate (render.py:57-70),
    (len(cameras) - 1) / (t_end - t_after_first) with the device synchronised before each clock read (nan for
    fewer than two cameras).  keep_images=False drops each image once rendered (images is then empty).
    antialiasing: render_view's."""
    images = []
    n, t1 = 0, 0.0
    for cam in cameras:
        img = render_view(cam, state, bg, antialiasing=antialiasing)["render"]
        if keep_images:
            images.append(img)
        n += 1
        if n == 1:
            _sync(state)
            t1 = _time.perf_counter()
    _sync(state)
    t2 = _time.perf_counter()
    fps = (n - 1) / (t2 - t1) if n > 1 and t2 > t1 else float("nan")
    return images, fps


def evaluate(state, views, bg, antialiasing=False):
    """{"psnr", "ssim"}: the means over `views` -- (camera, ground truth (3, H, W)) pairs -- of each image's PSNR
    and SSIM, as metrics.py forms them; the rendering is clamped to [0, 1].  antialiasing: render_view's."""
    from .losses import psnr
    vp, vs = [], []
    for cam, gt in views:
        img = render_view(cam, state, bg, antialiasing=antialiasing)["render"].clamp(0, 1).unsqueeze(0)
        gt = gt.to(img.device).unsqueeze(0)
        if img.is_cuda:
            from .kernels import ssim
        else:
            from .losses import ssim
        vp.append(psnr(img, gt).mean())
        vs.append(ssim(img, gt))
    if not vp:
        return {"psnr": float("nan"), "ssim": float("nan")}
    return {"psnr": float(torch.stack(vp).mean()), "ssim": float(torch.stack(vs).mean())}
