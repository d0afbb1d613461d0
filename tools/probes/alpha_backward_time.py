"""Cost of the opt-in alpha image and its gradient at the benchmark's configuration (diagnostic, GPU): P = 100k
Gaussians, 1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times).  tools/probes/depth_backward_time.py's
protocol: one process, HIP events around CALLS calls, median [min .. max] over ROUNDS rounds, the variants
alternating inside every round after a warm-up of each.

Reports, in microseconds per call:
  backward, colour only         _C.rasterize_gaussians_backward (gs4d_backward_ex)
  backward, depth               _C.rasterize_gaussians_backward_depth with the L1 depth gradient
  backward, aux, alpha          _C.rasterize_gaussians_backward_aux with the L1 mask gradient and no depth gradient
  backward, aux, depth + alpha  the same with both
  alpha image                   _C.alpha_image (gs4d_alpha_image), the forward's extra launch
  aux loss, HIP                 kernels.aux_loss_and_grad: both terms and both gradient images, two launches
  aux loss, torch               the torch formulation of the same two terms and gradients
and the full train step (arguments/dynerf, fused, one view) on a pair view against lambda_mask = lambda_depth = 0.5
on a (camera, gt, gt_depth, gt_mask) view, in milliseconds per step, alternating the same way.

--root DIR: import the packages of another checkout (its built tree), e.g. the parent commit's, whose two existing
backwards are then timed by the same script on the same box; rows a tree does not have are left out.
--small: P = 2,000 at 64x48 (a rehearsal of the script, not a measurement)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
import diff_gaussian_rasterization as dgr  # noqa: E402
from gs4d_train import config, kernels  # noqa: E402
from gs4d_train.gaussians import GaussianModel  # noqa: E402
from gs4d_train.render import render  # noqa: E402
from gs4d_train.synthetic import CONFIGS, make_point_cloud, make_scene, make_training_views, make_upstream_grad  # noqa: E402
from gs4d_train.train import depth_l1, train_step  # noqa: E402

CALLS, ROUNDS, STEPS = 10, 7, 5
HAS_AUX = hasattr(dgr._C, "rasterize_gaussians_backward_aux")


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(rows, n, rounds):
    for fn in rows.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in rows}
    for _ in range(rounds):
        for k, fn in rows.items():
            res[k].append(timed_us(fn, n))
    return res


def show(res, unit, div=1.0, digits=1):
    for k, v in res.items():
        v = [x / div for x in v]
        print(f"{k:34s} {statistics.median(v):10.{digits}f} {unit}  [{min(v):10.{digits}f} .. {max(v):10.{digits}f}]",
              flush=True)


def backward_rows(P, W, H, dev):
    s = make_scene(P, W, H, seed=0)
    t = lambda a: torch.tensor(np.asarray(a), device=dev)
    d = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix",
                              "campos")}
    e = torch.empty(0, device=dev)
    C = dgr._C
    nr, color, depth, radii, gb, bb, ib = C.rasterize_gaussians(
        d["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e, d["viewmatrix"],
        d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), H, W, d["shs"], 3, d["campos"], False, False)
    g_c = t(make_upstream_grad(color.cpu().numpy())[0])
    gt_d = depth * (1.0 + 0.1 * torch.randn_like(depth))
    g_d = torch.sign(depth - gt_d) / (H * W)
    head = (d["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], 1.0, e, d["viewmatrix"], d["projmatrix"],
            float(s["tanfovx"]), float(s["tanfovy"]))
    tail = (d["shs"], 3, d["campos"], gb, nr, bb, ib, False)
    rows = {
        "backward, colour only": lambda: C.rasterize_gaussians_backward(*head, g_c, *tail),
        "backward, depth": lambda: C.rasterize_gaussians_backward_depth(*head, g_c, g_d, *tail),
    }
    if HAS_AUX:
        alpha = C.alpha_image(ib, H, W)
        gt_m = (alpha + 0.2 * torch.randn_like(alpha)).clamp(0, 1)
        g_a = torch.sign(alpha - gt_m) / (H * W)

        def loss_torch():
            total, diff, n = depth_l1(depth, gt_d)
            dm = alpha - gt_m
            return total / n * 0.5 + dm.abs().mean() * 0.5, torch.sign(diff) * (0.5 / n), torch.sign(dm) * (0.5 / (H * W))
        rows.update({
            "backward, aux, alpha": lambda: C.rasterize_gaussians_backward_aux(*head, g_c, e, g_a, *tail),
            "backward, aux, depth + alpha": lambda: C.rasterize_gaussians_backward_aux(*head, g_c, g_d, g_a, *tail),
            "alpha image": lambda: C.alpha_image(ib, H, W),
            "aux loss, HIP": lambda: kernels.aux_loss_and_grad(depth, alpha, gt_d, gt_m, 0.5, 0.5),
            "aux loss, torch": loss_torch,
        })
    return rows, nr


def train_rows(P, W, H, dev):
    bg = torch.ones(3, device=dev)
    pts, cols = make_point_cloud(P, seed=0)
    pair = make_training_views(1, W, H, seed=1, device=dev)

    def model(points, lam):
        hyper, opt = config.dynerf()
        opt.lambda_depth = opt.lambda_mask = lam
        torch.manual_seed(0)
        g = GaussianModel(3, hyper, fused=True)
        g.create_from_pcd(points, cols, spatial_lr_scale=1.0, device=dev)
        g._deformation.deformation_net.grid.fused = True
        g._deformation.deformation_net.fused_heads = True
        g.training_setup(opt)
        g.active_sh_degree = 3
        return g, opt, hyper
    cases = [("train step, pair view", 0.0, pair)]
    if HAS_AUX:
        moved = (pts + np.random.default_rng(2).normal(0, 0.02, pts.shape)).astype(np.float32)
        other = model(moved, 0.0)[0]
        with torch.no_grad():
            pkg = render(pair[0][0], other, False, bg, alpha=True)
            quad = [(pair[0][0], pair[0][1], pkg["depth"].clone(), pkg["alpha"].clone())]
        del other, pkg
        cases.append(("train step, depth + mask view", 0.5, quad))
    rows = {}
    for label, lam, views in cases:
        g, opt, hyper = model(pts, lam)
        state = {"i": 3001}  # fine stage, statistics on, no densify / prune / reset iteration in range

        def one(g=g, opt=opt, hyper=hyper, views=views, state=state):
            train_step(g, views, opt, hyper, state["i"], bg)
            state["i"] += 1
        rows[label] = one
    return rows


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else CONFIGS["metric"]
    assert torch.cuda.is_available(), "alpha_backward_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows, nr = backward_rows(P, W, H, dev)
    print(f"alpha_backward_time: tree {ROOT} ({'with' if HAS_AUX else 'without'} the aux backward); P = {P}, {W}x{H}, "
          f"{nr} instances; {CALLS} calls x {ROUNDS} alternating rounds; median [min .. max]")
    res = alternate(rows, CALLS, ROUNDS)
    show(res, "us")
    med = {k: statistics.median(v) for k, v in res.items()}
    if HAS_AUX:
        print(f"aux alpha / colour-only backward: {med['backward, aux, alpha'] / med['backward, colour only']:.3f}; "
              f"aux depth + alpha / depth backward: {med['backward, aux, depth + alpha'] / med['backward, depth']:.3f}")
    res = alternate(train_rows(P, W, H, dev), STEPS, ROUNDS)
    show(res, "ms", 1e3, digits=3)
    if len(res) == 2:
        a, b = (statistics.median(v) for v in res.values())
        print(f"train step with / without the depth + mask view: {b / a:.3f}")


if __name__ == "__main__":
    main()
