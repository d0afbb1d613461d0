"""Cost of the opt-in absolute screen-space gradient at the benchmark's configuration (diagnostic, GPU): P = 100k
Gaussians, 1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times).

Reports, in microseconds per call (HIP events around CALLS calls, median [min .. max] over ROUNDS rounds; the
variants alternate inside every round of this one process, after a warm-up of each):
  backward, colour only         _C.rasterize_gaussians_backward (gs4d_backward_ex)
  backward, absgrad             _C.rasterize_gaussians_backward_absgrad with no depth gradient (the ABS walk)
  backward, depth               _C.rasterize_gaussians_backward_depth with the L1 depth gradient sign / (H W)
  backward, absgrad + depth     _C.rasterize_gaussians_backward_absgrad with that depth gradient (ABS + DEPTH)
and the full train step (arguments/dynerf, fused, one view) with densify_absgrad off and on, in milliseconds per
step, alternating the same way.  No pass bar is set on the absgrad rows: they are reported.
--small: P = 2,000 at 64x48 (a rehearsal of the script, not a measurement)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
import diff_gaussian_rasterization as dgr  # noqa: E402
from gs4d_train import config  # noqa: E402
from gs4d_train.gaussians import GaussianModel  # noqa: E402
from gs4d_train.synthetic import CONFIGS, make_point_cloud, make_scene, make_training_views, make_upstream_grad  # noqa: E402
from gs4d_train.train import train_step  # noqa: E402

CALLS, ROUNDS, STEPS = 10, 7, 5


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
    return {
        "backward, colour only": lambda: C.rasterize_gaussians_backward(*head, g_c, *tail),
        "backward, absgrad": lambda: C.rasterize_gaussians_backward_absgrad(*head, g_c, e, e, *tail),
        "backward, depth": lambda: C.rasterize_gaussians_backward_depth(*head, g_c, g_d, *tail),
        "backward, absgrad + depth": lambda: C.rasterize_gaussians_backward_absgrad(*head, g_c, g_d, e, *tail),
    }, nr


def train_rows(P, W, H, dev):
    bg = torch.ones(3, device=dev)
    pts, cols = make_point_cloud(P, seed=0)
    pair = make_training_views(1, W, H, seed=1, device=dev)
    rows = {}
    for label, flag in (("train step, densify_absgrad off", False), ("train step, densify_absgrad on", True)):
        hyper, opt = config.dynerf()
        opt.densify_absgrad = flag
        torch.manual_seed(0)
        g = GaussianModel(3, hyper, fused=True)
        g.create_from_pcd(pts, cols, spatial_lr_scale=1.0, device=dev)
        g._deformation.deformation_net.grid.fused = True
        g._deformation.deformation_net.fused_heads = True
        g.training_setup(opt)
        g.active_sh_degree = 3
        state = {"i": 3001}  # fine stage, statistics on, no densify / prune / reset iteration in range

        def one(g=g, opt=opt, hyper=hyper, state=state):
            train_step(g, pair, opt, hyper, state["i"], bg)
            state["i"] += 1
        rows[label] = one
    return rows


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else CONFIGS["metric"]
    assert torch.cuda.is_available(), "absgrad_backward_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows, nr = backward_rows(P, W, H, dev)
    print(f"absgrad_backward_time: P = {P}, {W}x{H}, {nr} instances; {CALLS} calls x {ROUNDS} alternating rounds; "
          f"median [min .. max]")
    res = alternate(rows, CALLS, ROUNDS)
    show(res, "us")
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"absgrad / colour-only backward: {med['backward, absgrad'] / med['backward, colour only']:.3f}; "
          f"absgrad + depth / depth backward: {med['backward, absgrad + depth'] / med['backward, depth']:.3f}")
    res = alternate(train_rows(P, W, H, dev), STEPS, ROUNDS)
    show(res, "ms", 1e3, digits=3)
    a, b = (statistics.median(v) for v in res.values())
    print(f"train step with / without densify_absgrad: {b / a:.3f}")


if __name__ == "__main__":
    main()
