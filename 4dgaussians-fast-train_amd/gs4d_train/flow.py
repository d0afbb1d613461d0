"""render_flow: an image of the 2-D motion of the deformed Gaussians, the first use of the rasterizer's feature
rendering (render(..., features=...)).

Per Gaussian the feature is its screen-space displacement between the camera's time t and t + dt, in pixels:
pix(m(t + dt)) - pix(m(t)), with m the deformed means and pix the rasterizer's own mapping of a mean to pixel
coordinates, ((ndc + 1) * (W, H) - 1) / 2 through the camera's full projection.  The image blends it with the weights
alpha * T of the frame at t (no background; divide by render(alpha=True)'s "alpha" for a per-pixel mean), and is
differentiable through both times: a loss on it reaches the deformation network (optical-flow supervision, motion
masks).  The reference has no such output.
"""
import torch

from .render import _time_float, _time_value, render

__all__ = ["render_flow", "pixel_coordinates"]


def pixel_coordinates(means3D, projmatrix, width, height):
    """(P, 2) pixel coordinates of `means3D` as the rasterizer maps them: p_hom = (m, 1) @ projmatrix, ndc = p_hom.xy /
    (p_hom.w + 1e-7), pix = ((ndc + 1) * (W, H) - 1) / 2."""
    p_hom = means3D @ projmatrix[:3] + projmatrix[3]
    ndc = p_hom[:, :2] / (p_hom[:, 3:4] + 0.0000001)
    size = torch.tensor([float(width), float(height)], dtype=means3D.dtype, device=means3D.device)
    return ((ndc + 1.0) * size - 1.0) * 0.5


def _camera_tensors(camera, dev, camera_tensors):
    # render()'s choice of the view matrix and the full projection
    if camera_tensors is not None:
        return camera_tensors[0], camera_tensors[1]
    if hasattr(camera, "on_device"):
        view_m, proj_m, _ = camera.on_device(dev)
        return view_m, proj_m
    return camera.world_view_transform.to(dev), camera.full_proj_transform.to(dev)


def flow_rows(camera, pc, means_t, dt, camera_tensors=None):
    """The (P, 2) per-Gaussian displacement in pixels from the deformed means at the camera's time (`means_t`) to
    those at time + dt, which take a positions-only pass through the deformation (the field and the position head);
    zero for a Gaussian that is not in front of the camera at time + dt (view depth <= 0.2, mark_visible's rule).
    The pass at time + dt always runs the plain fp32 layers, whatever path render() is configured with for `means_t`:
    against the fused fp32 heads the two ends differ by fp32 rounding only, but with mlp_dtype="bf16" `means_t` carries
    the bf16 heads' error and the other end does not, so a static Gaussian then shows a flow of the order of that
    error times the focal length over its depth -- supervise flow on an fp32 model, or subtract render_flow(dt=0)."""
    xyz = pc.get_xyz
    dev = xyz.device
    view_m, proj_m = _camera_tensors(camera, dev, camera_tensors)
    W, H = int(camera.image_width), int(camera.image_height)
    net = pc._deformation.deformation_net
    if net.args.no_dx:
        means_dt = xyz
    else:
        t2 = _time_value(_time_float(_time_float(camera.time) + float(dt)), dev).expand(xyz.shape[0], 1)
        # the position head alone, as plain layers: the fused heads block packs the active heads' weights for the
        # full set, which a one-head call would re-pack
        means_dt = xyz + net.pos_deform(net.feature_out(net.grid(xyz, t2)))
    disp = pixel_coordinates(means_dt, proj_m, W, H) - pixel_coordinates(means_t, proj_m, W, H)
    depth_dt = means_dt @ view_m[:3, 2] + view_m[3, 2]
    return torch.where((depth_dt > 0.2).unsqueeze(1), disp, torch.zeros_like(disp))


def render_flow(camera, pc, bg, dt, stage="fine", **render_kwargs):
    """render()'s package with "flow" (2, H, W): channel 0 the x and channel 1 the y displacement in pixels over
    `dt`, blended with the frame's weights.  In the coarse stage nothing moves and the flow is exactly zero.
    render_kwargs go to render() (pipe_debug, scaling_modifier, depth_grad, alpha, absgrad, antialiasing,
    camera_tensors); `features` is taken by the flow and camera_grad is not available with it."""
    if "features" in render_kwargs:
        raise ValueError("render_flow: the feature image is the flow; render other features with render()")
    pipe_debug = render_kwargs.pop("pipe_debug", False)
    if "coarse" in stage:
        rows = torch.zeros((pc.get_xyz.shape[0], 2), dtype=torch.float32, device=pc.get_xyz.device)
    else:
        cam_t = render_kwargs.get("camera_tensors")
        rows = lambda means_t: flow_rows(camera, pc, means_t, dt, cam_t)
    pkg = render(camera, pc, pipe_debug, bg, stage=stage, features=rows, **render_kwargs)
    dict.__setitem__(pkg, "flow", dict.pop(pkg, "features"))
    return pkg
