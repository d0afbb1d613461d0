"""Cost of the blend-weight importance pass next to the forward it follows (diagnostic, GPU): P = 100k Gaussians,
1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times).

Reports, the rows alternated inside every round of this one process after a warm-up of each:
  the forward's `render` stage          libgs4d's own event bracket (_C.set_profiling(1), _C.last_timings()): the blend
                                        kernel whose walk the pass replays, microseconds, median [min .. max] over
                                        CALLS x ROUNDS calls
  forward call                          HIP events around CALLS calls of _C.rasterize_gaussians, microseconds per call
  importance pass                       HIP events around CALLS calls of _C.gaussian_importance on one forward's state
                                        (its three launches: the walk, the segmented reduce, the finishing pass; the
                                        calls queue faster than they run, so this is device time per call)
  forward call + importance pass        what diff_gaussian_rasterization.gaussian_importance runs per view
and the ratio of the pass to the `render` stage.  No pass bar is set: the rows are reported.
--small: P = 2,000 at 64x48 (a rehearsal of the script, not a measurement)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
import diff_gaussian_rasterization as dgr  # noqa: E402
from gs4d_train.synthetic import CONFIGS, make_scene  # noqa: E402

CALLS, ROUNDS = 20, 9


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def show(label, v):
    print(f"{label:34s} {statistics.median(v):10.1f} us  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else CONFIGS["metric"]
    assert torch.cuda.is_available(), "importance_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    C = dgr._C
    s = make_scene(P, W, H, seed=0)
    t = lambda a: torch.tensor(np.asarray(a), device=dev)
    d = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix",
                              "campos")}
    e = torch.empty(0, device=dev)

    def fwd():
        return C.rasterize_gaussians(d["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e,
                                     d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), H, W,
                                     d["shs"], 3, d["campos"], False, False)
    nr, _, _, radii, gb, bb, ib = fwd()

    def imp():
        return C.gaussian_importance(gb, bb, ib, nr, P, H, W)

    def both():
        f = fwd()
        return C.gaussian_importance(f[4], f[5], f[6], f[0], P, H, W)
    wsum, wmax, count = imp()
    print(f"importance_time: P = {P}, {W}x{H}, {nr} instances; {int((count > 0).sum())} Gaussians blend, "
          f"{int(count.long().sum())} blended pairs; {CALLS} calls x {ROUNDS} alternating rounds; median [min .. max]")
    rows = {"forward call": fwd, "importance pass": imp, "forward call + importance pass": both}
    for fn in rows.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in rows}
    render = []
    for _ in range(ROUNDS):
        C.set_profiling(1)
        try:
            for _ in range(CALLS):
                fwd()
                render += [ms * 1e3 for name, ms in C.last_timings() if name == "render"]
        finally:
            C.set_profiling(0)
        for k, fn in rows.items():
            res[k].append(timed_us(fn, CALLS))
    show("render stage of the forward", render)
    for k, v in res.items():
        show(k, v)
    print(f"importance pass / render stage: {statistics.median(res['importance pass']) / statistics.median(render):.2f}")


if __name__ == "__main__":
    main()
