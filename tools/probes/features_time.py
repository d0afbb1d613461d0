"""Cost of the fused feature rendering next to the composition it replaces (diagnostic, GPU): P = 100k Gaussians,
1352x1014 (synthetic.CONFIGS["metric"], the scene bench.py times), C in {2, 8, 16, 32}.

For each C, the rows alternated inside every round of this one process after a warm-up of each, HIP events around
CALLS calls, microseconds per call, median [min .. max] over ROUNDS rounds:
  fused forward        _C.rasterize_features on one finished forward's state
  fused backward       _C.rasterize_features_backward on that state (every gradient)
  composition forward  ceil(C / 3) calls of _C.rasterize_gaussians with three channels as colors_precomp
  composition backward ceil(C / 3) calls of _C.rasterize_gaussians_backward on those forwards' states
The cost condition of DESIGN 10.14: at C >= 8 the fused forward + backward must lie below the composition's in the
same run, the fused maximum below the composition's minimum; C = 2 is reported.  Exit status 1 when it is missed.
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

CALLS, ROUNDS = 5, 7
CHANNELS = (2, 8, 16, 32)


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def show(label, v):
    print(f"  {label:34s} {statistics.median(v):10.1f} us  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else CONFIGS["metric"]
    assert torch.cuda.is_available(), "features_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    C = dgr._C
    s = make_scene(P, W, H, seed=0)
    t = lambda a: torch.tensor(np.asarray(a), device=dev)
    d = {k: t(s[k]) for k in ("means3D", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos")}
    e = torch.empty(0, device=dev)
    bg = torch.zeros(3, device=dev)
    tx, ty = float(s["tanfovx"]), float(s["tanfovy"])
    rng = np.random.default_rng(1)

    def forward(colors):
        return C.rasterize_gaussians(bg, d["means3D"], colors, d["opacities"], d["scales"], d["rotations"], 1.0, e,
                                     d["viewmatrix"], d["projmatrix"], tx, ty, H, W, e, 0, d["campos"], False, False)

    def backward(colors, fwd, grad):
        return C.rasterize_gaussians_backward(bg, d["means3D"], fwd[3], colors, d["scales"], d["rotations"], 1.0, e,
                                              d["viewmatrix"], d["projmatrix"], tx, ty, grad, e, 0, d["campos"], fwd[4],
                                              fwd[0], fwd[5], fwd[6], False)
    print(f"features_time: P = {P}, {W}x{H}, FEATURE_CHUNK = {C.FEATURE_CHUNK}; {CALLS} calls x {ROUNDS} alternating "
          f"rounds; median [min .. max]")
    ok = True
    for Cn in CHANNELS:
        f = t(rng.normal(0, 1, (P, Cn)).astype(np.float32))
        g = t(rng.normal(0, 1, (Cn, H, W)).astype(np.float32))
        groups = []
        for a in range(0, Cn, 3):
            n = min(3, Cn - a)
            col = torch.zeros(P, 3, device=dev)
            col[:, :n] = f[:, a:a + n]
            gp = torch.zeros(3, H, W, device=dev)
            gp[:n] = g[a:a + n]
            groups.append((col, gp, forward(col)))
        state = groups[0][2]

        def fused_fwd():
            return C.rasterize_features(f, state[4], state[0], state[5], state[6], P, H, W)

        def fused_bwd():
            return C.rasterize_features_backward(f, g, d["means3D"], state[3], d["scales"], d["rotations"], 1.0, e,
                                                 d["viewmatrix"], d["projmatrix"], tx, ty, state[4], state[0], state[5],
                                                 state[6], e, False, True)

        def comp_fwd():
            return [forward(col) for col, _, _ in groups]

        def comp_bwd():
            return [backward(col, fwd, gp) for col, gp, fwd in groups]
        rows = {"fused forward": fused_fwd, "fused backward": fused_bwd, "composition forward": comp_fwd,
                "composition backward": comp_bwd}
        for fn in rows.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        res = {k: [] for k in rows}
        for _ in range(ROUNDS):
            for k, fn in rows.items():
                res[k].append(timed_us(fn, CALLS))
        print(f"C = {Cn} ({len(groups)} composition calls each way, {state[0]} instances)")
        for k, v in res.items():
            show(k, v)
        fused = [a + b for a, b in zip(res["fused forward"], res["fused backward"])]
        comp = [a + b for a, b in zip(res["composition forward"], res["composition backward"])]
        show("fused forward + backward", fused)
        show("composition forward + backward", comp)
        verdict = "below" if max(fused) < min(comp) else "NOT below"
        print(f"  fused / composition (medians) {statistics.median(fused) / statistics.median(comp):.2f}; fused maximum "
              f"{verdict} the composition's minimum", flush=True)
        if Cn >= 8 and not max(fused) < min(comp):
            ok = False
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
