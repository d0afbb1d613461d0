"""Device time of the (F, W) = (48, 128) kernels at the HyperNeRF preset (diagnostic, GPU): P = 100k Gaussians,
arguments/hypernerf/default.py hyper-parameters (three grid levels, F = 48, W = 128, heads pos / scales / rot).

Four legs, each an A/B that alternates round by round in this one process after a warm-up of both sides; HIP events
on the stream around REPS calls, microseconds per call, median [min .. max] over the rounds.  A difference counts
when it exceeds that min .. max spread.
  (a) first layer, forward + backward: _FeatureReLU (gs4d_feature_relu_forward / _backward) against the Linear + ReLU
      autograd formulation it replaces (deformation.Linear: nn.Linear with the split-K weight gradient, as
      Deformation.feature_out holds it; x needs a gradient, as the field's features do)
  (b) a frame's deformation through infer.state_at_time: the fused path against state.fused = False (the torch
      formulation this shape ran before gs4d_deform_infer served it)
  (c) one fine-stage train_step (1352x1014, one view): this tree against the parent's formulation, i.e.
      _FeatureReLU.shapes without (48, 128), which sends the first layer to Linear + ReLU
  (d) gs4d_feature_relu_backward alone at (48, 128) and, for scale, at (32, 128)
--small: P = 2,000 at 64x48 (a rehearsal of the script, not a measurement)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
from gs4d_train import _C, config, deformation, infer  # noqa: E402
from gs4d_train.gaussians import GaussianModel  # noqa: E402
from gs4d_train.synthetic import make_point_cloud, make_training_views  # noqa: E402
from gs4d_train.train import train_step  # noqa: E402

ROUNDS = 7
PARENT_SHAPES = ((32, 128), (64, 64), (32, 64))


def per_call_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ab(title, rows, reps, warm=5):
    """rows: {name: fn}; every fn warmed up, then timed once per round, the rows alternating within each round"""
    for fn in rows.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in rows}
    for _ in range(ROUNDS):
        for k, fn in rows.items():
            res[k].append(per_call_us(fn, reps))
    print(f"{title}  ({reps} calls per round, {ROUNDS} alternating rounds; us per call: median [min .. max])")
    for k, v in res.items():
        print(f"  {k:44s} {statistics.median(v):10.1f}  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)
    return res


def model(P, dev, opt=None):
    hyper, _ = config.hypernerf()
    torch.manual_seed(0)
    g = GaussianModel(3, hyper, fused=True)
    pts, cols = make_point_cloud(P, seed=0)
    g.create_from_pcd(pts, cols, spatial_lr_scale=1.0, device=dev)
    g.active_sh_degree = 3
    net = g._deformation.deformation_net
    net.grid.fused = net.fused_heads = True
    if opt is not None:
        g.training_setup(opt)
    else:
        with torch.no_grad():  # a field that moves the Gaussians: the planes off their initial values
            for level in net.grid.grids:
                for p in level:
                    p.copy_(torch.rand_like(p) * 0.4 + 0.1)
    return g, hyper


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else (100_000, 1352, 1014)
    assert torch.cuda.is_available(), "hypernerf_shape_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"hypernerf_shape_time: P = {P}, hypernerf preset (F = 48, W = 128, heads 3/3/4), {W}x{H}")

    # (a) the first layer, forward + backward
    torch.manual_seed(1)
    lin = deformation.Linear(48, 128).to(dev)
    x = (torch.rand(P, 48, 6, device=dev) * 0.4 + 0.1).prod(-1).requires_grad_(True)
    up = torch.randn(P, 128, device=dev)
    params = [x, lin.weight, lin.bias]

    def fused_layer():
        return torch.autograd.grad(deformation._FeatureReLU.apply(x, lin.weight, lin.bias), params, up)

    def torch_layer():
        return torch.autograd.grad(torch.relu(lin(x)), params, up)
    ab("(a) first layer forward + backward", {"_FeatureReLU (HIP)": fused_layer, "Linear + ReLU (torch autograd)": torch_layer}, 50)
    d = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused_layer(), torch_layer()))
    print(f"  largest |fused - torch| gradient difference, of its tensor's max: {d:.2e}")

    # (d) the backward kernel alone
    def bwd_rows(fin):
        w = torch.randn(128, fin, device=dev) * 0.2
        xx = torch.randn(P, fin, device=dev)
        h = _C.feature_relu_forward(xx, w, torch.zeros(128, device=dev))[0]
        return lambda: _C.feature_relu_backward(up, h, xx, w)
    ab("(d) gs4d_feature_relu_backward alone", {"(48, 128)": bwd_rows(48), "(32, 128)": bwd_rows(32)}, 50)

    # (b) a frame's deformation
    g, hyper = model(P, dev)
    state = infer.prepare(g)
    assert state.fused, "the HyperNeRF preset must run the fused path"
    served, infer._SHAPES = infer._SHAPES, PARENT_SHAPES
    try:
        unfused = infer.prepare(g)
    finally:
        infer._SHAPES = served
    assert not unfused.fused
    res = ab("(b) infer.state_at_time", {"fused (gs4d_deform_infer)": lambda: infer.state_at_time(state, 0.37),
                                         "state.fused = False (torch)": lambda: infer.state_at_time(unfused, 0.37)}, 50)
    d = max(float((a - b).abs().max()) for a, b in zip(infer.state_at_time(state, 0.37), infer.state_at_time(unfused, 0.37)))
    print(f"  largest |fused - unfused| over the five outputs: {d:.3e}")
    del res, state, unfused, g

    # (c) one fine-stage train step
    _, opt = config.hypernerf()
    g, hyper = model(P, dev, opt)
    views = make_training_views(1, W, H, seed=1, device=dev)
    bg = torch.ones(3, device=dev)
    it = {"i": 3001}  # fine stage, densification statistics on, no densify / prune / reset iteration in range

    def step(shapes):
        def one():
            deformation._FeatureReLU.shapes = shapes
            try:
                train_step(g, views, opt, hyper, it["i"], bg)
            finally:
                deformation._FeatureReLU.shapes = served_train
            it["i"] += 1
        return one
    served_train = deformation._FeatureReLU.shapes
    ab("(c) train_step, fine stage, one view", {"this tree (fused first layer)": step(served_train),
                                               "parent formulation (Linear + ReLU)": step(PARENT_SHAPES)}, 10, warm=3)


if __name__ == "__main__":
    main()
