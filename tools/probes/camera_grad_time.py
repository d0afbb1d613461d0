"""Cost of the opt-in camera gradient at the benchmark's configuration (diagnostic, GPU): P = 100k Gaussians,
1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times).

Reports, with the option off and on, alternated inside every round of this one process after a warm-up of each:
  the backward's stages   libgs4d's own event brackets (_C.set_profiling(1), _C.last_timings()), microseconds per
                          stage, median [min .. max] over CALLS x ROUNDS calls; `gaussian_backward` holds the new
                          device code: the camera-on instantiation of the per-Gaussian kernel (its 27 values, the
                          wave and workgroup sums, one row per workgroup) and the launch that adds the rows
  the whole backward      HIP events around CALLS calls of _C.rasterize_gaussians_backward_aa (off) /
                          _C.rasterize_gaussians_backward_camera (on), microseconds per call
The option-off rows run the code objects of a build without the option (tools/kernel_diff.py), so their spread is
that build's; a build whose `_C` lacks the camera entry reports the off rows alone.
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
from gs4d_train.synthetic import CONFIGS, make_scene, make_upstream_grad  # noqa: E402

CALLS, ROUNDS = 10, 7
STAGES = ("render_backward", "contrib_reduce", "gaussian_backward")


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def show(res, unit="us"):
    for k, v in res.items():
        print(f"{k:40s} {statistics.median(v):10.1f} {unit}  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)


def backward_rows(P, W, H, dev):
    """{label: backward call} for the option off and on, after one forward of the metric scene"""
    s = make_scene(P, W, H, seed=0)
    t = lambda a: torch.tensor(np.asarray(a), device=dev)
    d = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix",
                              "campos")}
    e = torch.empty(0, device=dev)
    C = dgr._C
    nr, color, depth, radii, gb, bb, ib = C.rasterize_gaussians(
        d["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e, d["viewmatrix"], d["projmatrix"],
        float(s["tanfovx"]), float(s["tanfovy"]), H, W, d["shs"], 3, d["campos"], False, False)
    g_c = t(make_upstream_grad(color.cpu().numpy())[0])
    args = (d["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], 1.0, e, d["viewmatrix"], d["projmatrix"],
            float(s["tanfovx"]), float(s["tanfovy"]), g_c, e, e, d["shs"], 3, d["campos"], gb, nr, bb, ib, False,
            d["opacities"], False, False)
    rows = {"off": lambda: C.rasterize_gaussians_backward_aa(*args)}
    if hasattr(C, "rasterize_gaussians_backward_camera"):
        rows["on"] = lambda: C.rasterize_gaussians_backward_camera(*args)
    return rows, nr


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else CONFIGS["metric"]
    assert torch.cuda.is_available(), "camera_grad_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows, nr = backward_rows(P, W, H, dev)
    print(f"camera_grad_time: P = {P}, {W}x{H}, num_rendered = {nr}, {torch.cuda.get_device_name(0)}; "
          f"{CALLS} calls x {ROUNDS} rounds, off / on alternating", flush=True)
    for fn in rows.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    C = dgr._C
    stages = {f"{st}, camera_grad {k}": [] for st in STAGES for k in rows}
    C.set_profiling(1)
    try:
        for _ in range(ROUNDS):
            for k, fn in rows.items():
                for _ in range(CALLS):
                    fn()
                    for name, ms in C.last_timings():
                        if name in STAGES:
                            stages[f"{name}, camera_grad {k}"].append(ms * 1e3)
    finally:
        C.set_profiling(0)
    show(stages)
    whole = {f"whole backward, camera_grad {k}": [] for k in rows}
    for _ in range(ROUNDS):
        for k, fn in rows.items():
            whole[f"whole backward, camera_grad {k}"].append(timed_us(fn, CALLS))
    show(whole)


if __name__ == "__main__":
    main()
