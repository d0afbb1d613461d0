"""Cost of the opt-in antialiased rasterization at the benchmark's configuration (diagnostic, GPU): P = 100k
Gaussians, 1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times).

Reports, with the option off and on, alternated inside every round of this one process after a warm-up of each:
  the forward's and the backward's stages  libgs4d's own event brackets (_C.set_profiling(1), _C.last_timings()),
                                           microseconds per stage, median [min .. max] over CALLS x ROUNDS calls:
                                           `preprocess` and `gaussian_backward` hold the new device code; `render`
                                           and `render_backward` see the smaller opacity through the exact tile
                                           culling (fewer emitted instances)
  forward and backward, whole calls        HIP events around CALLS calls of _C.rasterize_gaussians_aa /
                                           _C.rasterize_gaussians_backward_aa, microseconds per call
  the full train step                      arguments/dynerf, fused, one view, opt.antialiasing off and on,
                                           milliseconds per step
No pass bar is set: the rows are reported.
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
STAGES = ("preprocess", "binning", "render", "render_backward", "contrib_reduce", "gaussian_backward")


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


def raster_rows(P, W, H, dev):
    """{label: (forward, backward)} for the option off and on, on the metric scene"""
    s = make_scene(P, W, H, seed=0)
    t = lambda a: torch.tensor(np.asarray(a), device=dev)
    d = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix",
                              "campos")}
    e = torch.empty(0, device=dev)
    C = dgr._C
    rows = {}
    for label, aa in (("off", False), ("on", True)):
        def fwd(aa=aa):
            return C.rasterize_gaussians_aa(
                d["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e, d["viewmatrix"],
                d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), H, W, d["shs"], 3, d["campos"], False,
                False, aa)
        nr, color, depth, radii, gb, bb, ib = fwd()
        g_c = t(make_upstream_grad(color.cpu().numpy())[0])

        def bwd(aa=aa, g_c=g_c, radii=radii, gb=gb, nr=nr, bb=bb, ib=ib):
            return C.rasterize_gaussians_backward_aa(
                d["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], 1.0, e, d["viewmatrix"],
                d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), g_c, e, e, d["shs"], 3, d["campos"], gb, nr,
                bb, ib, False, d["opacities"], aa, False)
        rows[label] = (fwd, bwd, nr)
    return rows


def stage_times(rows, n, rounds):
    """{stage: {label: [us]}} from the library's event brackets, the labels alternating"""
    C = dgr._C
    out = {st: {k: [] for k in rows} for st in STAGES}
    C.set_profiling(1)
    try:
        for _ in range(rounds):
            for k, (fwd, bwd, _) in rows.items():
                for _ in range(n):
                    fwd()
                    for name, ms in C.last_timings():
                        if name in out:
                            out[name][k].append(ms * 1e3)
                    bwd()
                    for name, ms in C.last_timings():
                        if name in out:
                            out[name][k].append(ms * 1e3)
    finally:
        C.set_profiling(0)
    return out


def train_rows(P, W, H, dev):
    bg = torch.ones(3, device=dev)
    pts, cols = make_point_cloud(P, seed=0)
    pair = make_training_views(1, W, H, seed=1, device=dev)
    rows = {}
    for label, flag in (("train step, antialiasing off", False), ("train step, antialiasing on", True)):
        hyper, opt = config.dynerf()
        opt.antialiasing = flag
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
    assert torch.cuda.is_available(), "antialias_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows = raster_rows(P, W, H, dev)
    print(f"antialias_time: P = {P}, {W}x{H}, {rows['off'][2]} instances (num_rendered, the same off and on: "
          f"{rows['on'][2]}); {CALLS} calls x {ROUNDS} alternating rounds; median [min .. max]")
    for k, (fwd, bwd, _) in rows.items():  # warm-up
        for _ in range(3):
            fwd(), bwd()
    torch.cuda.synchronize()
    for st, by in stage_times(rows, CALLS, ROUNDS).items():
        show({f"{st}, antialiasing {k}": v for k, v in by.items()}, "us")
    calls = {}
    for k, (fwd, bwd, _) in rows.items():
        calls[f"forward call, antialiasing {k}"] = fwd
        calls[f"backward call, antialiasing {k}"] = bwd
    show(alternate(calls, CALLS, ROUNDS), "us")
    res = alternate(train_rows(P, W, H, dev), STEPS, ROUNDS)
    show(res, "ms", 1e3, digits=3)
    a, b = (statistics.median(v) for v in res.values())
    print(f"train step with / without antialiasing: {b / a:.3f}")


if __name__ == "__main__":
    main()
