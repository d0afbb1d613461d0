"""One training iteration of the reference's train.py (scene_reconstruction, :144-387), restated.

train_step() renders a batch of views through the deformation field and the rasterizer, takes the
L1 loss (+ HexPlane regularisers in the fine stage, + D-SSIM when lambda_dssim != 0), back-propagates,
sums the viewspace gradients over the views, updates the densification statistics, densifies /
prunes / resets opacity on the reference's schedule, and steps the optimizer.  What it leaves out
is logging and I/O: the reference's per-step host syncs for the progress bar (loss.item(), psnr)
and the NaN check that re-execs the program (:255-257) are not part of a training step's work.

With `data_parallel=True` the views of the batch are sharded over the torch.distributed ranks
(gs4d_train.dp): each rank renders its share, and the parameter gradients, viewspace gradients,
radii and visibility are reduced so every replica takes the single-process step.

Depth supervision (this build's opt-in, no reference counterpart): with opt.lambda_depth != 0 a view given as
(camera, gt_image, gt_depth) adds lambda_depth * mean over the valid pixels (gt_depth > 0) of
|depth - gt_depth| to the loss, and is rendered with depth_grad=True so the term reaches the Gaussians.

Mask supervision (opt-in as well): with opt.lambda_mask != 0 a view given as (camera, gt_image, gt_depth or None,
gt_mask) is rendered with alpha=True and adds lambda_mask * mean |alpha - gt_mask|, alpha being the rasterizer's
accumulated-alpha image 1 - T_final.  Such a view's depth and mask terms come from one fused kernel pair on the
fused path (kernels.aux_loss_and_grad); views without a mask take the code they took before.

Absolute-gradient densification (opt-in, AbsGS): with opt.densify_absgrad every view is rendered with absgrad=True
and the densification statistics accumulate the norm of the views' summed `viewspace_points.absgrad[:, :2]` --
per Gaussian the sum over its pixels of |the pixel's pull on the 2-D mean| -- in place of the norm of the signed
sum `viewspace_points.grad`, which cancels for a large blurry Gaussian pulled both ways.  The thresholds are the
user's: AbsGS roughly doubles densify_grad_threshold_* (0.0004 for the reference's 0.0002).

Antialiased rasterization (opt-in, Mip-Splatting's 2-D filter): with opt.antialiasing every view is rendered with
antialiasing=True, the opacity compensated for the rasterizer's 0.3 px^2 low-pass; a model trained so is rendered
so (infer.render_view / render_set / evaluate take the same switch).

Pose refinement (opt-in): with a gs4d_train.pose.PoseRefiner passed as `pose` and opt.pose_lr > 0, every view is
rendered through the refiner's camera tensors with camera_grad=True, so the rasterizer's camera gradient reaches the
per-camera deltas, which an Adam of their own (lr = opt.pose_lr) steps after the Gaussians' optimizer.  The deltas'
gradients are not reduced across ranks, so a refiner does not combine with data_parallel.

Local rigidity (opt-in): with a gs4d_train.rigidity.Rigidity passed as `rigidity` and opt.lambda_rigid != 0, the fine
stage adds lambda_rigid * the isometry term between the canonical means and each view's deformed means over an exact
K-NN graph of the canonical means (rigidity.py); the views are rendered with return_means=True for it.

MCMC densification (opt-in, 3DGS-MCMC): with opt.densify_strategy == "mcmc" the clone / split / prune heuristic, its
statistics and the opacity reset do not run.  The step adds mcmc_opacity_reg * mean(opacity) + mcmc_scale_reg *
mean(scale) to the loss (its gradient joins the parameters' after the backward, gs4d_train.mcmc.regulariser_and_grad),
and after the optimizer relocates the dead Gaussians (opacity <= mcmc_min_opacity) onto live ones and grows the set by
5 % up to mcmc_cap_max on the densification schedule, then adds the opacity-gated position noise of every step
(gs4d_train/mcmc.py).  Every draw is a function of (mcmc_seed, iteration).
"""
import functools

import torch

from . import dp
from .losses import l1_loss_torch


def depth_l1(depth, gt_depth):
    """(sum over the valid pixels of |depth - gt_depth|, masked difference, number of valid pixels (>= 1));
    gt_depth is (1, H, W) or (H, W), a pixel is valid where gt_depth > 0"""
    gt = gt_depth.reshape(depth.shape)
    valid = gt > 0
    diff = torch.where(valid, depth - gt, torch.zeros_like(depth))
    return diff.abs().sum(), diff, valid.sum().clamp(min=1)


def train_step(gaussians, views, opt, hyper, iteration, background, stage="fine", fused_loss=None,
               data_parallel=False, render_fn=None, pose=None, rigidity=None):
    """views: list of (camera, gt_image (3, H, W)), (camera, gt_image, gt_depth (1, H, W) or (H, W)) or
    (camera, gt_image, gt_depth or None, gt_mask (1, H, W) or (H, W), floats in [0, 1]); the depth is read only
    when opt.lambda_depth != 0 and the mask only when opt.lambda_mask != 0.  Returns the (detached) batch loss
    tensor.

    render_fn(camera, gaussians, debug, bg, stage=...) -> render()'s dict; defaults to
    gs4d_train.render.render (the HIP rasterizer).  The multi-process CPU tests pass a torch stand-in.  It is
    called with depth_grad=True and / or alpha=True only for the views that need them, and with absgrad=True for
    every view when opt.densify_absgrad is on (its viewspace_points must then carry .absgrad after the backward),
    and with antialiasing=True for every view when opt.antialiasing is on.

    pose: a PoseRefiner; with opt.pose_lr > 0 every view is rendered with camera_grad=True and
    camera_tensors=pose.tensors(camera), and the refiner's deltas are stepped by their own Adam after the Gaussians'
    optimizer.  With pose=None or opt.pose_lr == 0 nothing of this runs.

    rigidity: a gs4d_train.rigidity.Rigidity; with opt.lambda_rigid != 0, in the fine stage, every view is rendered
    with return_means=True and the step adds lambda_rigid * isometry(get_xyz, means3D(t)) per view, scaled like the
    depth term, over the graph rigidity.graph_for(gaussians, iteration) gives (asked once, before the renders; a
    densification inside the step makes it rebuild at the next one).  The term reads the render's own deformed means:
    no second deformation pass.  With rigidity=None or opt.lambda_rigid == 0 nothing of this runs.

    opt.densify_strategy == "mcmc": add_densification_stats, densify, prune and reset_opacity are skipped; the
    regulariser's value joins the returned loss and its gradient the parameters' (after the backward and, in a
    data-parallel step, after the all-reduce: it depends on the parameters alone, which every replica holds); after
    optimizer.step(), for densify_from_iter < iteration < densify_until_iter with iteration % densification_interval
    == 0, mcmc.relocate then mcmc.grow run, and every step ends with mcmc.inject_noise at step_scale = mcmc_noise_lr *
    the xyz group's current learning rate.  It composes with data_parallel=True with no broadcast: the draws come from a
    counter-based generator keyed by (opt.mcmc_seed, iteration, row), the same on every replica.  With "default" (or
    an opt without the field) nothing of this runs."""
    strategy = getattr(opt, "densify_strategy", "default")
    if strategy not in ("default", "mcmc"):
        raise ValueError(f"train_step: opt.densify_strategy must be \"default\" or \"mcmc\", got {strategy!r}")
    mcmc_on = strategy == "mcmc"
    if render_fn is None:
        from .render import render as render_fn
    posing = pose is not None and float(getattr(opt, "pose_lr", 0.0)) > 0.0
    if posing:
        if data_parallel:
            raise ValueError("train_step: pose refinement does not combine with data_parallel=True: the pose "
                             "gradients are not reduced across ranks (out of scope)")
        plain_render_fn = render_fn

        def render_fn(cam, *args, **kw):
            return plain_render_fn(cam, *args, camera_grad=True, camera_tensors=pose.tensors(cam), **kw)
    fused = gaussians.fused if fused_loss is None else fused_loss
    gaussians.update_learning_rate(iteration)
    if iteration % 1000 == 0:
        gaussians.oneupSHdegree()
    mine = dp.shard_views(len(views)) if data_parallel else list(range(len(views)))
    images, gts, radii_list, vis_list, vs_list = [], [], [], [], []
    lambda_depth = getattr(opt, "lambda_depth", 0.0)
    lambda_mask = getattr(opt, "lambda_mask", 0.0)
    depths, gt_depths = [], []  # of the views that carry a gt depth, when lambda_depth != 0
    masked = []  # (depth or None, gt_depth or None, alpha, gt_mask) of the views that carry a mask, when lambda_mask != 0
    densify_absgrad = bool(getattr(opt, "densify_absgrad", False))
    if densify_absgrad:
        render_fn = functools.partial(render_fn, absgrad=True)
    if bool(getattr(opt, "antialiasing", False)):
        render_fn = functools.partial(render_fn, antialiasing=True)
    lambda_rigid = float(getattr(opt, "lambda_rigid", 0.0))
    rigid_graph = None
    if lambda_rigid != 0 and rigidity is not None and stage == "fine":
        rigid_graph = rigidity.graph_for(gaussians, iteration)
        render_fn = functools.partial(render_fn, return_means=True)
    means_list = []  # the views' deformed means, when the rigidity term is on
    for v in mine:
        cam, gt = views[v][0], views[v][1]
        has_depth = lambda_depth != 0 and len(views[v]) > 2 and views[v][2] is not None
        if lambda_mask != 0 and len(views[v]) > 3 and views[v][3] is not None:
            if has_depth:
                pkg = render_fn(cam, gaussians, False, background, stage=stage, depth_grad=True, alpha=True)
                masked.append((pkg["depth"], views[v][2], pkg["alpha"], views[v][3]))
            else:
                pkg = render_fn(cam, gaussians, False, background, stage=stage, alpha=True)
                masked.append((None, None, pkg["alpha"], views[v][3]))
        elif has_depth:
            pkg = render_fn(cam, gaussians, False, background, stage=stage, depth_grad=True)
            depths.append(pkg["depth"])
            gt_depths.append(views[v][2])
        else:
            pkg = render_fn(cam, gaussians, False, background, stage=stage)
        if rigid_graph is not None:
            if "means3D" not in pkg:
                raise RuntimeError("opt.lambda_rigid: render_fn's package carries no \"means3D\"; render_fn must honour "
                                   "return_means=True (gs4d_train.render.render does)")
            means_list.append(pkg["means3D"])
        images.append(pkg["render"].unsqueeze(0))
        gts.append(gt.unsqueeze(0))
        radii_list.append(pkg["radii"].unsqueeze(0))
        vis_list.append(pkg)  # its visibility_filter (radii > 0) is read only where needed below
        vs_list.append(pkg["viewspace_points"])
    P = gaussians.get_xyz.shape[0]
    dev = gaussians.get_xyz.device
    # train.py:221-228 batches the views with torch.cat and reduces radii / visibility over them; with one view
    # per rank those are the view's own tensors (no copies, no reductions)
    one = len(mine) == 1
    if one:
        # the fused statistics filter by radii > 0 inside their kernel (visibility_filter's definition)
        radii = radii_list[0][0]
        visibility_filter = None if (gaussians.fused and not data_parallel) else vis_list[0]["visibility_filter"]
    else:
        vis_list = [pk["visibility_filter"].unsqueeze(0) for pk in vis_list]
        radii = torch.cat(radii_list, 0).max(dim=0).values if radii_list else torch.zeros(P, dtype=torch.int32,
                                                                                       device=dev)
        visibility_filter = torch.cat(vis_list).any(dim=0) if vis_list else torch.zeros(P, dtype=torch.bool,
                                                                                      device=dev)
    image_grad = None  # fused path: the image loss's gradient, formed with its value (L1: one pass; + D-SSIM: two)
    if images:
        image_tensor = images[0] if one else torch.cat(images, 0)
        gt_image_tensor = gts[0] if one else torch.cat(gts, 0)
        # the batch mean over all views: each rank holds len(mine) of len(views)
        share = len(mine) / len(views) if data_parallel else 1.0
        if fused and opt.lambda_dssim == 0:
            # loss = L1 * share (+ the regulariser, deferred below) is linear in the L1, so
            # loss.backward() deposits exactly image.backward(sign / N * share): value and gradient in one
            # pass (gs4d_l1_loss_grad), no L1 autograd node
            from .kernels import l1_loss_and_grad
            Ll1, image_grad = l1_loss_and_grad(image_tensor, gt_image_tensor[:, :3, :, :], share)
            loss = Ll1 * share if data_parallel else Ll1
        elif fused:
            # the same with D-SSIM: loss = (L1 + lambda * (1 - ssim)) * share, both values and the complete image
            # gradient in two launches (gs4d_l1_dssim_loss_grad)
            from .kernels import l1_dssim_loss_and_grad
            Ll1, ssim_value, image_grad = l1_dssim_loss_and_grad(image_tensor, gt_image_tensor[:, :3, :, :],
                                                                 opt.lambda_dssim, share)
            loss = Ll1 + opt.lambda_dssim * (1.0 - ssim_value)
            loss = loss * share if data_parallel else loss
        else:
            Ll1 = l1_loss_torch(image_tensor, gt_image_tensor[:, :3, :, :])
            loss = Ll1 * share if data_parallel else Ll1
    else:
        loss = torch.zeros((), device=dev)
    depth_grads = None
    if depths:
        # lambda_depth * (batch mean over this rank's views of the per-view valid-pixel mean) * share, like the L1
        scale = lambda_depth * share / len(mine)
        if image_grad is not None:
            # fused path: the term's value and its gradient formed explicitly (one H x W pass per view in torch)
            depth_grads = []
            with torch.no_grad():
                for d, gd in zip(depths, gt_depths):
                    total, diff, n = depth_l1(d, gd)
                    loss = loss + total / n * scale
                    depth_grads.append(torch.sign(diff) * (scale / n))
        else:
            for d, gd in zip(depths, gt_depths):
                total, _, n = depth_l1(d, gd)
                loss = loss + total / n * scale
    aux_tensors, aux_grads = [], []
    if masked:
        # per view: lambda_depth * valid-pixel mean |depth - gt_depth| + lambda_mask * mean |alpha - gt_mask|, scaled
        # like the depth term above
        scale = share / len(mine)
        for d, gd, a, gm in masked:
            if image_grad is not None:
                # fused path: the view's value and both gradient images in two launches (gs4d_aux_loss_grad)
                from .kernels import aux_loss_and_grad
                value, g_d, g_a = aux_loss_and_grad(d, a, None if gd is None else gd.reshape(d.shape),
                                                    gm.reshape(a.shape), lambda_depth * scale, lambda_mask * scale)
                loss = loss + value
                if d is not None:
                    aux_tensors.append(d)
                    aux_grads.append(g_d)
                aux_tensors.append(a)
                aux_grads.append(g_a)
            else:
                if d is not None:
                    total, _, n = depth_l1(d, gd)
                    loss = loss + total / n * (lambda_depth * scale)
                loss = loss + (a - gm.reshape(a.shape)).abs().mean() * (lambda_mask * scale)
    rigid_tensors, rigid_grads = [], []
    if means_list:
        # per view: lambda_rigid * isometry(canonical means, the view's deformed means), scaled like the depth term
        from .rigidity import isometry_loss, isometry_loss_and_grad
        scale = lambda_rigid * share / len(mine)
        xyz = gaussians.get_xyz
        if image_grad is not None:
            # fused path: the value and both explicit gradients in one pass per view (gs4d_isometry_loss_grad)
            xyz_grad = None
            for m in means_list:
                value, g_a, g_b = isometry_loss_and_grad(xyz, m, rigid_graph, scale)
                loss = loss + value
                if m.requires_grad:
                    rigid_tensors.append(m)
                    rigid_grads.append(g_b)
                xyz_grad = g_a if xyz_grad is None else xyz_grad + g_a
            if xyz.requires_grad:
                rigid_tensors.append(xyz)
                rigid_grads.append(xyz_grad)
        else:
            for m in means_list:
                loss = loss + isometry_loss(xyz, m, rigid_graph) * scale
    reg_w = (hyper.time_smoothness_weight, hyper.l1_time_planes, hyper.plane_tv_weight)
    reg_scale = 1.0 / dp.world() if data_parallel else 1.0
    reg_deferred = False
    if stage == "fine" and hyper.time_smoothness_weight != 0:
        if fused:
            # the regulariser depends only on the planes: after the backward one pass over them adds its
            # gradient to the planes' gradients and gives its value, which joins the reported loss
            reg_deferred = True
        else:
            reg = gaussians.compute_regulation(*reg_w)
            loss = loss + reg * reg_scale
    if opt.lambda_dssim != 0 and images and not fused:
        from .losses import ssim
        loss = loss + opt.lambda_dssim * (1.0 - ssim(image_tensor, gt_image_tensor)) * (
            len(mine) / len(views) if data_parallel else 1.0)
    # a data-parallel rank with no view of the batch (len(views) < world) and no regulariser has a
    # constant loss: nothing to back-propagate, its gradients are the zeros filled in below
    if image_grad is not None:
        if image_tensor.requires_grad and (aux_tensors or rigid_tensors):
            # one backward pass: each view's rasterizer backward takes its colour, depth and alpha gradients together,
            # and the deformation the rigidity term's gradient at the deformed means with the rasterizer's
            torch.autograd.backward([image_tensor] + depths + aux_tensors + rigid_tensors,
                                    [image_grad] + (depth_grads or []) + aux_grads + rigid_grads)
        elif image_tensor.requires_grad and depth_grads:
            # one backward pass: each view's rasterizer backward takes its colour and depth gradients together
            torch.autograd.backward([image_tensor] + depths, [image_grad] + depth_grads)
        elif image_tensor.requires_grad:
            image_tensor.backward(image_grad)
    elif loss.requires_grad:
        loss.backward()
    if reg_deferred:
        if reg_scale == 1.0:
            # loss.detach() + value, the add inside the regulariser's own launch
            loss = gaussians.add_regulation_grad(*reg_w, scale=reg_scale, with_value=True, base=loss.detach())
        else:
            loss = loss.detach() + gaussians.add_regulation_grad(*reg_w, scale=reg_scale, with_value=True) * reg_scale
    if len(vs_list) == 1 and vs_list[0].grad is not None:
        viewspace_grad = vs_list[0].grad
    else:
        viewspace_grad = torch.zeros_like(gaussians.get_xyz)
        for t in vs_list:
            if t.grad is not None:
                viewspace_grad = viewspace_grad + t.grad
    if densify_absgrad:
        # the densification signal: the views' absolute gradients, summed like their signed ones (which still
        # reach the parameters through autograd; only the statistics read this tensor)
        abs_list = []
        for t in vs_list:
            if t.grad is not None:  # this view's rasterizer backward ran
                if getattr(t, "absgrad", None) is None:
                    raise RuntimeError("opt.densify_absgrad: render_fn's viewspace_points carries no .absgrad after the "
                                       "backward; render_fn must honour absgrad=True (gs4d_train.render.render does)")
                abs_list.append(t.absgrad)
        if len(abs_list) == 1:
            viewspace_grad = abs_list[0]
        else:
            viewspace_grad = torch.zeros_like(gaussians.get_xyz)
            for t in abs_list:
                viewspace_grad = viewspace_grad + t
    # the returned loss: a view when nothing writes it later (the data-parallel all-reduce sums in place)
    loss_out = loss.detach().reshape(1)
    if data_parallel:
        loss_out = loss_out.clone()
    if data_parallel and dp.world() > 1:
        # a parameter gets a gradient on every replica iff some rank produced one (a rank without views
        # produces none); parameters no rank touched keep grad None, so the optimizer skips them as the
        # single-process step does (their Adam step counts stay in step)
        params = [p for g in gaussians.optimizer.param_groups for p in g["params"]]
        has = torch.tensor([p.grad is not None for p in params], dtype=torch.int32, device=dev)
        torch.distributed.all_reduce(has, op=torch.distributed.ReduceOp.MAX)
        params = [p for p, h in zip(params, has.tolist()) if h]
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        vis_i = visibility_filter.to(torch.int32)
        dp.allreduce_sum_([p.grad for p in params] + [viewspace_grad, loss_out])
        torch.distributed.all_reduce(radii, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(vis_i, op=torch.distributed.ReduceOp.MAX)
        visibility_filter = vis_i.bool()
    if mcmc_on:
        from . import mcmc
        loss_out = loss_out + mcmc.regulariser_and_grad(gaussians, float(opt.mcmc_opacity_reg), float(opt.mcmc_scale_reg))
    with torch.no_grad():
        if mcmc_on:
            pass  # no statistics, no clone / split / prune, no opacity reset: relocation and growth follow the optimizer
        elif iteration < opt.densify_until_iter:
            gaussians.add_densification_stats(viewspace_grad, visibility_filter, radii)
            if stage == "coarse":
                opacity_threshold = opt.opacity_threshold_coarse
                densify_threshold = opt.densify_grad_threshold_coarse
            else:
                opacity_threshold = opt.opacity_threshold_fine_init - iteration * (
                    opt.opacity_threshold_fine_init - opt.opacity_threshold_fine_after) / opt.densify_until_iter
                densify_threshold = opt.densify_grad_threshold_fine_init - iteration * (
                    opt.densify_grad_threshold_fine_init - opt.densify_grad_threshold_after) / opt.densify_until_iter
            extent = getattr(gaussians, "cameras_extent", 1.0)
            if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0 and P < 360000:
                size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                # the split's random offsets are rank 0's on every replica only in a data-parallel step
                gaussians.data_parallel_step = bool(data_parallel)
                try:
                    gaussians.densify(densify_threshold, opacity_threshold, extent, size_threshold)
                finally:
                    gaussians.data_parallel_step = False
            if iteration > opt.pruning_from_iter and iteration % opt.pruning_interval == 0 and \
                    gaussians.get_xyz.shape[0] > 200000:
                size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                gaussians.prune(densify_threshold, opacity_threshold, extent, size_threshold)
            if iteration % opt.opacity_reset_interval == 0:
                gaussians.reset_opacity()
        if iteration < opt.iterations:
            gaussians.optimizer.step()
            gaussians.optimizer.zero_grad(set_to_none=True)
            if posing:
                pose_opt = _pose_optimizer(pose, float(opt.pose_lr))
                pose_opt.step()
                pose_opt.zero_grad(set_to_none=True)
            if mcmc_on:
                seed, min_opacity = int(opt.mcmc_seed), float(opt.mcmc_min_opacity)
                if opt.densify_from_iter < iteration < opt.densify_until_iter and \
                        iteration % opt.densification_interval == 0:
                    mcmc.relocate(gaussians, seed, iteration, min_opacity)
                    mcmc.grow(gaussians, seed, iteration, int(opt.mcmc_cap_max), min_opacity)
                xyz_lr = next(g["lr"] for g in gaussians.optimizer.param_groups if g["name"] == "xyz")
                mcmc.inject_noise(gaussians, float(opt.mcmc_noise_lr) * float(xyz_lr), seed, iteration)
    return loss_out[0]


def _pose_optimizer(pose, lr):
    """the refiner's own Adam over (rot, trans), made on first use and kept on the refiner"""
    pose_opt = getattr(pose, "optimizer", None)
    if pose_opt is None:
        pose_opt = pose.optimizer = torch.optim.Adam(pose.parameters(), lr=lr)
    for group in pose_opt.param_groups:
        group["lr"] = lr
    return pose_opt
