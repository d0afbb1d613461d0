"""MI355X drop-in for the `diff_gaussian_rasterization` extension API.

Public surface identical to the reference package
(submodules/depth-diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py:12-220):

  GaussianRasterizationSettings  NamedTuple, same field order (:157-169)
  GaussianRasterizer             nn.Module with forward(...) and markVisible(...) (:171-220)
  rasterize_gaussians            functional entry (:21-42)
  _RasterizeGaussians            torch.autograd.Function (:44-155)

so gaussian_renderer/__init__.py and train.py run unchanged.  Three opt-in extensions, off by default:
depth_grad=True (rasterize_gaussians, GaussianRasterizer) selects _RasterizeGaussiansDepth, whose backward
also back-propagates the depth image's gradient, which the reference drops (:100-101); alpha=True selects
_RasterizeGaussiansAux, which also returns the accumulated-alpha image 1 - T_final (1, H, W) as a fourth,
differentiable output (the reference returns no such image, :98); absgrad=True selects the _RasterizeGaussians*Abs
Functions, whose backward also leaves the absolute screen-space gradient (AbsGS; gsplat's `absgrad`) in
`means2D.absgrad`, a (P, 3) tensor overwritten by every backward call.  A fourth, antialiasing=True, is a value
of the forward and not another Function: the opacity blended is o * sqrt(max(2.5e-5, det S / det(S + 0.3 I))) for
the projected covariance S (Mip-Splatting's 2-D filter; gsplat's rasterize_mode="antialiased"), and the backward
carries that factor's gradient into the covariance; radii and the binning do not change.  A fifth, camera_grad=True,
makes raster_settings' viewmatrix, projmatrix and campos inputs of the same Function, so the ones that require grad
receive dL/dviewmatrix, dL/dprojmatrix and dL/dcampos (pose refinement; gsplat's viewmats.grad): the forward is
unchanged and the backward runs _C.rasterize_gaussians_backward_camera, whose other gradients are bit for bit
those of the flag-off call.  A sixth, features=F with a (P, C) float32 tensor, is one more input of the same Function:
the feature image (C, H, W), sum_i w_i f_i with the forward's blend weights and no background, is appended as the last
output (_C.rasterize_features, one more walk over the state the forward left) and its gradient reaches F and the
geometry inputs through _C.rasterize_features_backward; the other outputs and their backward keep their bits.  Beside
the Functions, gaussian_importance(...) runs one forward without a graph and
returns what each Gaussian deposited in it: per Gaussian the sum and the maximum of its blend weights alpha * T and the
number of pixels it reached (the scores score-based pruning ranks by).  The compute runs in libgs4d (HIP
kernels for gfx950) through the `_C` binding built in-tree by build_ext.py; importing this package
without the built extension raises ImportError -- there is no CPU fallback.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C  # noqa: F401  (fails loudly when the HIP extension is missing)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians",
           "_RasterizeGaussiansDepth", "_RasterizeGaussiansAux", "_RasterizeGaussiansAuxDepth",
           "_RasterizeGaussiansAbs", "_RasterizeGaussiansAbsDepth", "_RasterizeGaussiansAuxAbs",
           "_RasterizeGaussiansAuxDepthAbs"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _snapshot(args):
    """Host copies of the call arguments, taken before the call in debug mode (reference :17-19)."""
    return tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)


def _invoke(fn, args, debug, dump_name, stage):
    """Run a `_C` entry point; in debug mode dump the arguments if it raises (reference :83-90,132-139)."""
    if not debug:
        return fn(*args)
    saved = _snapshot(args)
    try:
        return fn(*args)
    except Exception:
        torch.save(saved, dump_name)
        print(f"\nAn error occured in {stage}. Please forward {dump_name} for debugging.")
        raise


def _check_features(features, means3D, camera_grad):
    if camera_grad:
        raise ValueError("features: the feature image has no camera gradient; camera_grad=True is not supported with it")
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.dtype != torch.float32:
        raise ValueError("features must be a 2-D float32 tensor (P, C)")
    if features.shape[0] != means3D.shape[0]:
        raise ValueError(f"features must have one row per Gaussian: {features.shape[0]} rows for {means3D.shape[0]}")
    if features.shape[1] == 0:
        raise ValueError("features must have at least one channel (C >= 1)")
    if features.device != means3D.device:
        raise ValueError("features must be on the means' device")


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, depth_grad=False, alpha=False, absgrad=False, antialiasing=False,
                        camera_grad=False, features=None):
    """(color, radii, depth), or with alpha=True (color, radii, depth, alpha).  absgrad=True: the backward also
    assigns `means2D.absgrad` (P, 3): per Gaussian the sum over its pixels of |the pixel's term of means2D.grad|
    in x and y (column 2 is 0), where means2D.grad holds the signed sum.  antialiasing=True: the footprint-
    compensated opacity (module docstring) is blended, through the same Function.  camera_grad=True:
    raster_settings.viewmatrix / .projmatrix / .campos follow the switch as inputs and receive their gradients.
    features (P, C) float32: the feature image (C, H, W), sum_i w_i f_i with the forward's weights and no
    background, is appended as the last output; the other outputs keep their bits.  Its gradient reaches `features`
    and the geometry inputs; `means2D.absgrad` stays the colour path's alone.  ValueError with camera_grad=True."""
    fn = _FUNCTIONS[bool(depth_grad), bool(alpha), bool(absgrad)]
    if features is not None:  # the features ride the same Function as one more input after the switch
        _check_features(features, means3D, camera_grad)
        return fn.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, bool(antialiasing), features)
    if camera_grad:
        s = raster_settings
        return fn.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, bool(antialiasing), s.viewmatrix, s.projmatrix, s.campos)
    if antialiasing:
        return fn.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, True)
    return fn.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                    raster_settings)


def _zero_image(channels, s, like):
    return torch.zeros((channels, s.image_height, s.image_width), dtype=torch.float32, device=like.device)


def _forward(ctx, variant, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
             raster_settings, antialiasing=False, *extra):
    # extra: (viewmatrix, projmatrix, campos), raster_settings' own tensors as inputs of the Function (camera_grad),
    # or (features,), the rows of the opt-in feature image
    camera = extra if len(extra) == 3 else ()
    features = extra[0] if len(extra) == 1 else None
    depth_grad, alpha, absgrad = variant
    s = raster_settings
    # positional order of _C.rasterize_gaussians (rasterize_points.h:18-38)
    args = (s.bg, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree,
            s.campos, s.prefiltered, s.debug)
    if antialiasing:  # the same arguments, then the switch; the backward needs the raw opacities
        num_rendered, color, depth, radii, geom_buf, binning_buf, img_buf = _invoke(
            _C.rasterize_gaussians_aa, args + (True,), s.debug, "snapshot_fw.dump", "forward")
    else:
        num_rendered, color, depth, radii, geom_buf, binning_buf, img_buf = _invoke(
            _C.rasterize_gaussians, args, s.debug, "snapshot_fw.dump", "forward")
    ctx.antialiasing = bool(antialiasing)
    ctx.aa_input = len(extra) > 0 or bool(antialiasing)  # the switch was an input of the Function
    ctx.camera_grad = len(camera) > 0
    ctx.has_features = features is not None
    ctx.variant = variant
    ctx.raster_settings = s
    ctx.num_rendered = num_rendered
    # radii are integers, and a gradient that did not arrive means "none" to the backward: autograd need not
    # build zero gradients before calling it
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom_buf,
                          binning_buf, img_buf, *((opacities,) if antialiasing or camera else ()),
                          *((features,) if features is not None else ()))
    if absgrad:
        ctx.absgrad_target = means2D  # the caller's tensor: the backward assigns its .absgrad
    feature_image = ()
    if features is not None:  # one more walk over the state the forward left, which it does not change
        if means3D.shape[0] == 0:
            feature_image = (_zero_image(features.shape[1], s, means3D),)
        else:
            feature_image = (_C.rasterize_features(features, geom_buf, num_rendered, binning_buf, img_buf,
                                                   means3D.shape[0], s.image_height, s.image_width),)
    if not alpha:
        return (color, radii, depth) + feature_image
    if means3D.shape[0] == 0:  # nothing was drawn and there is no image state to read
        alpha_image = _zero_image(1, s, means3D)
    else:
        alpha_image = _C.alpha_image(img_buf, s.image_height, s.image_width)
    return (color, radii, depth, alpha_image) + feature_image


def _features_backward(ctx, grad_features):
    """The feature image's gradients: (g_means3D, g_means2D, g_opacities, g_scales, g_rotations, g_cov3D), each None
    when no geometry input requires grad (the entry then skips the geometry stages), and g_features."""
    s = ctx.raster_settings
    _, means3D, scales, rotations, cov3Ds_precomp, radii, _, geom_buf, binning_buf, img_buf = ctx.saved_tensors[:10]
    features = ctx.saved_tensors[-1]
    if means3D.shape[0] == 0:
        return (None,) * 6 + (torch.zeros_like(features),)
    geometry = any(ctx.needs_input_grad[i] for i in (0, 1, 4, 5, 6, 7))
    opacities = ctx.saved_tensors[10] if ctx.antialiasing else torch.empty(0, dtype=torch.float32, device=means3D.device)
    g_feat, g_means2D, g_opac, g_means3D, g_cov3D, g_scales, g_rot = _C.rasterize_features_backward(
        features, grad_features, means3D, radii, scales, rotations, s.scale_modifier, cov3Ds_precomp, s.viewmatrix,
        s.projmatrix, s.tanfovx, s.tanfovy, geom_buf, ctx.num_rendered, binning_buf, img_buf, opacities,
        ctx.antialiasing, geometry)
    if not geometry:
        return (None,) * 6 + (g_feat,)
    return g_means3D, g_means2D, g_opac, g_scales, g_rot, g_cov3D, g_feat


def _backward(ctx, grad_out_color, grad_depth, grad_alpha, grad_features=None):
    if not ctx.variant[0]:  # depth_grad off: no gradient flows from the depth image, like the reference (:100-101)
        grad_depth = None
    if ctx.has_features:  # camera_grad is excluded with features: the inputs end (..., switch, features)
        base = (None,) * 9
        if not (grad_out_color is None and grad_depth is None and grad_alpha is None):
            base = _backward_images(ctx, grad_out_color, grad_depth, grad_alpha)[:9]
        if grad_features is None:
            return base + (None, None)
        f3, f2, fo, fs, fr, fc, g_feat = _features_backward(ctx, grad_features)
        add = lambda a, b: b if a is None else (a if b is None else a + b)
        g_means3D, g_means2D, g_sh, g_colors, g_opacities, g_scales, g_rotations, g_cov3D = base[:8]
        return (add(g_means3D, f3), add(g_means2D, f2), g_sh, g_colors, add(g_opacities, fo), add(g_scales, fs),
                add(g_rotations, fr), add(g_cov3D, fc), None, None, g_feat if ctx.needs_input_grad[10] else None)
    return _backward_images(ctx, grad_out_color, grad_depth, grad_alpha)


def _backward_images(ctx, grad_out_color, grad_depth, grad_alpha):
    depth_grad, alpha, absgrad = ctx.variant
    s = ctx.raster_settings
    # the switch itself, when it was an input, and the three camera tensors after it
    extra = ((None,) if ctx.aa_input else ()) + ((None,) * 3 if ctx.camera_grad else ())
    if grad_out_color is None and grad_depth is None and grad_alpha is None:
        return (None,) * 9 + extra  # only images without a gradient path were used: nothing flows back
    (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom_buf, binning_buf,
     img_buf) = ctx.saved_tensors[:10]
    # the entry and its upstream images, which follow grad_out_color in its argument list
    tail = ()
    if ctx.antialiasing or ctx.camera_grad:  # one entry for every combination: empty tensors and False stand for "off"
        entry = _C.rasterize_gaussians_backward_camera if ctx.camera_grad else _C.rasterize_gaussians_backward_aa
        if grad_out_color is None:
            grad_out_color = _zero_image(3, s, means3D)
        none = torch.empty(0, dtype=torch.float32, device=means3D.device)
        grads = (grad_out_color, none if grad_depth is None else grad_depth, none if grad_alpha is None else grad_alpha)
        tail = (ctx.saved_tensors[10], ctx.antialiasing, bool(absgrad))
    elif alpha or absgrad:  # an empty tensor stands for "no such gradient"
        entry = _C.rasterize_gaussians_backward_absgrad if absgrad else _C.rasterize_gaussians_backward_aux
        if grad_out_color is None:
            grad_out_color = _zero_image(3, s, means3D)
        none = torch.empty(0, dtype=torch.float32, device=means3D.device)
        grads = (grad_out_color, none if grad_depth is None else grad_depth, none if grad_alpha is None else grad_alpha)
    elif depth_grad:
        entry = _C.rasterize_gaussians_backward_depth
        if grad_out_color is None:
            grad_out_color = _zero_image(3, s, means3D)
        if grad_depth is None:
            grad_depth = _zero_image(1, s, means3D)
        grads = (grad_out_color, grad_depth)
    else:
        entry = _C.rasterize_gaussians_backward
        grads = (grad_out_color,)
    # positional order of _C.rasterize_gaussians_backward (rasterize_points.h:40-62)
    args = (s.bg, means3D, radii, colors_precomp, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, *grads, sh, s.sh_degree, s.campos,
            geom_buf, ctx.num_rendered, binning_buf, img_buf, s.debug, *tail)
    out = _invoke(entry, args, s.debug, "snapshot_bw.dump", "backward")
    if absgrad:
        ctx.absgrad_target.absgrad = out[8]  # overwritten per backward call (gsplat's convention)
    g_means2D, g_colors, g_opacities, g_means3D, g_cov3D, g_sh, g_scales, g_rotations = out[:8]
    if ctx.camera_grad:  # only the camera tensors that require grad take theirs
        extra = (None,) + tuple(g if need else None for g, need in zip(out[9:12], ctx.needs_input_grad[10:13]))
    return (g_means3D, g_means2D, g_sh, g_colors, g_opacities, g_scales, g_rotations, g_cov3D, None) + extra


def _variant(depth_grad, alpha, absgrad):
    """(forward, backward) of the Function with these options, over the shared bodies above."""
    variant = (depth_grad, alpha, absgrad)

    def forward(ctx, *inputs):
        return _forward(ctx, variant, *inputs)

    def backward(ctx, grad_out_color, grad_radii, grad_depth, *rest):
        # rest: the alpha image's gradient (alpha=True), then the feature image's (features given)
        grad_alpha = rest[0] if alpha and rest else None
        return _backward(ctx, grad_out_color, grad_depth, grad_alpha, rest[-1] if ctx.has_features else None)

    return staticmethod(forward), staticmethod(backward)


class _RasterizeGaussians(torch.autograd.Function):
    forward, backward = _variant(False, False, False)


class _RasterizeGaussiansDepth(torch.autograd.Function):
    """_RasterizeGaussians whose backward also takes the depth image's gradient (opt-in: depth_grad=True)."""
    forward, backward = _variant(True, False, False)


class _RasterizeGaussiansAux(torch.autograd.Function):
    """_RasterizeGaussians that also returns the alpha image 1 - T_final (opt-in: alpha=True), whose gradient flows
    back through _C.rasterize_gaussians_backward_aux; the depth image's gradient is dropped, as by default."""
    forward, backward = _variant(False, True, False)


class _RasterizeGaussiansAuxDepth(torch.autograd.Function):
    """_RasterizeGaussiansAux whose backward takes the depth image's gradient too (alpha=True, depth_grad=True)."""
    forward, backward = _variant(True, True, False)


class _RasterizeGaussiansAbs(torch.autograd.Function):
    """_RasterizeGaussians whose backward also assigns means2D.absgrad (opt-in: absgrad=True)."""
    forward, backward = _variant(False, False, True)


class _RasterizeGaussiansAbsDepth(torch.autograd.Function):
    """_RasterizeGaussiansDepth with means2D.absgrad (absgrad=True, depth_grad=True)."""
    forward, backward = _variant(True, False, True)


class _RasterizeGaussiansAuxAbs(torch.autograd.Function):
    """_RasterizeGaussiansAux with means2D.absgrad (absgrad=True, alpha=True)."""
    forward, backward = _variant(False, True, True)


class _RasterizeGaussiansAuxDepthAbs(torch.autograd.Function):
    """_RasterizeGaussiansAuxDepth with means2D.absgrad (absgrad=True, alpha=True, depth_grad=True)."""
    forward, backward = _variant(True, True, True)


# (depth_grad, alpha, absgrad) -> the Function rasterize_gaussians applies
_FUNCTIONS = {(False, False, False): _RasterizeGaussians, (True, False, False): _RasterizeGaussiansDepth,
              (False, True, False): _RasterizeGaussiansAux, (True, True, False): _RasterizeGaussiansAuxDepth,
              (False, False, True): _RasterizeGaussiansAbs, (True, False, True): _RasterizeGaussiansAbsDepth,
              (False, True, True): _RasterizeGaussiansAuxAbs, (True, True, True): _RasterizeGaussiansAuxDepthAbs}


def _empty_if_none(t):
    # "not provided" travels as an empty tensor (reference :197-207)
    return torch.Tensor([]) if t is None else t


@torch.no_grad()
def gaussian_importance(means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                        cov3D_precomp=None, raster_settings=None, antialiasing=False):
    """(weight_sum, weight_max, pixel_count, radii) of one view: one forward (antialiased with antialiasing=True)
    and _C.gaussian_importance over the state it left.  Per Gaussian i, over the pixels the forward blended it
    into, with w = alpha * T the weight the forward multiplied into the colour: weight_sum[i] = sum w (float32, a
    fixed summation order), weight_max[i] = max w and pixel_count[i] = the number of those pixels (int32), the
    last two exact; zeros for a Gaussian the view culls.  No graph is built and nothing here is differentiable."""
    if raster_settings is None:
        raise ValueError("gaussian_importance: raster_settings is required")
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    have_sr = scales is not None or rotations is not None
    if (cov3D_precomp is None and (scales is None or rotations is None)) or (have_sr and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    s = raster_settings
    P = means3D.shape[0]
    if P == 0:
        f = torch.empty(0, dtype=torch.float32, device=means3D.device)
        i = torch.empty(0, dtype=torch.int32, device=means3D.device)
        return f, f.clone(), i, i.clone()
    args = (s.bg, means3D, _empty_if_none(colors_precomp), opacities, _empty_if_none(scales),
            _empty_if_none(rotations), s.scale_modifier, _empty_if_none(cov3D_precomp), s.viewmatrix, s.projmatrix,
            s.tanfovx, s.tanfovy, s.image_height, s.image_width, _empty_if_none(shs), s.sh_degree, s.campos,
            s.prefiltered, s.debug)
    if antialiasing:
        num_rendered, _, _, radii, geom_buf, binning_buf, img_buf = _C.rasterize_gaussians_aa(*args, True)
    else:
        num_rendered, _, _, radii, geom_buf, binning_buf, img_buf = _C.rasterize_gaussians(*args)
    weight_sum, weight_max, pixel_count = _C.gaussian_importance(geom_buf, binning_buf, img_buf, num_rendered, P,
                                                                 s.image_height, s.image_width)
    return weight_sum, weight_max, pixel_count, radii


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings, depth_grad=False, alpha=False, absgrad=False, antialiasing=False,
                 camera_grad=False):
        super().__init__()
        self.camera_grad = camera_grad  # opt-in: the settings' camera tensors receive their gradients
        self.antialiasing = antialiasing  # opt-in: the footprint-compensated opacity o * s is blended
        self.absgrad = absgrad  # opt-in: the backward assigns means2D.absgrad (_RasterizeGaussians*Abs)
        self.raster_settings = raster_settings
        self.depth_grad = depth_grad  # opt-in: the depth image's gradient flows back (_RasterizeGaussiansDepth)
        self.alpha = alpha  # opt-in: forward also returns the alpha image 1 - T_final (_RasterizeGaussiansAux)

    def markVisible(self, positions):
        """Near-plane visibility mask of `positions` for this camera (reference :176-185)."""
        with torch.no_grad():
            s = self.raster_settings
            return _C.mark_visible(positions, s.viewmatrix, s.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None):
        # argument exclusivity rules and messages of the reference (:191-195)
        if (shs is None) == (colors_precomp is None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        have_sr = scales is not None or rotations is not None
        if (cov3D_precomp is None and (scales is None or rotations is None)) or (have_sr and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, _empty_if_none(shs), _empty_if_none(colors_precomp), opacities,
                                   _empty_if_none(scales), _empty_if_none(rotations), _empty_if_none(cov3D_precomp),
                                   self.raster_settings, depth_grad=self.depth_grad, alpha=self.alpha,
                                   absgrad=self.absgrad, antialiasing=self.antialiasing,
                                   **({"camera_grad": True} if self.camera_grad else {}),
                                   **({"features": features} if features is not None else {}))
