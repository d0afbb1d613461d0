"""Per-frame device time of the inference path at the metric shape (diagnostic, GPU): P = 100k Gaussians,
1352x1014, arguments/dynerf hyper-parameters (F = 32, W = 128, five heads), 50 distinct timestamps.

Reports, in microseconds per frame (HIP events around the 50 frames, median over the rounds):
  state_at_time            gs4d_train.infer: points + field over the packed planes + gs4d_deform_infer
    its three launches     each timed alone over the same 50 timestamps
  parent formulation       what render() runs under no_grad without this module: pc._deformation(...) with the
                           fused field on (HIP field incl. its per-call pack, eleven torch Linears) + the activations
  render_view              state_at_time + the rasterizer
and render_set's FPS over the 50 cameras.  The two formulations alternate round by round in this one process, after
a warm-up of every shape.  --small: P = 2,000 at 64x48 (a rehearsal of the script, not a measurement)."""
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
from gs4d_train import _C, config, infer  # noqa: E402
from gs4d_train.gaussians import GaussianModel  # noqa: E402
from gs4d_train.render import _time_float, _time_value  # noqa: E402
from gs4d_train.synthetic import look_at_camera, make_point_cloud  # noqa: E402

FRAMES, ROUNDS = 50, 7


def per_frame_us(fn, times):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in times:
        fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / len(times) * 1e3


def main():
    small = "--small" in sys.argv
    P, W, H = (2000, 64, 48) if small else (100_000, 1352, 1014)
    assert torch.cuda.is_available(), "infer_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    hyper, _ = config.dynerf()
    torch.manual_seed(0)
    g = GaussianModel(3, hyper, fused=True)
    pts, cols = make_point_cloud(P, seed=0)
    g.create_from_pcd(pts, cols, spatial_lr_scale=1.0, device=dev)
    g.active_sh_degree = 3
    net = g._deformation.deformation_net
    net.grid.fused = True
    net.fused_heads = True
    with torch.no_grad():  # a field that moves the Gaussians: the planes off their initial values
        for level in net.grid.grids:
            for p in level:
                p.copy_(torch.rand_like(p) * 0.4 + 0.1)
    times = [i / (FRAMES - 1) for i in range(FRAMES)]
    cams = [look_at_camera(W, H, (4.0 * math.sin(0.02 * i), 0.3, -4.0 * math.cos(0.02 * i)), time=t)
            for i, t in enumerate(times)]
    bg = torch.ones(3, device=dev)
    state = infer.prepare(g)
    assert state.fused, "the metric configuration must run the fused path"
    xyz = state.xyz
    tcol = lambda t: _time_value(_time_float(t), dev).expand(P, 1)
    pts0 = _C.hexplane_points(xyz, tcol(0.5), state.aabb)
    feat0 = _C.hexplane_forward_packed(pts0, state.packed, state.plane_f, state.plane_w, state.plane_h, state.order)

    def parent(t):
        with torch.no_grad():
            m3, sc, rot, op, sh = g._deformation(g.get_xyz, g._scaling, g._rotation, g._opacity, g.get_features, tcol(t))
            return m3, torch.exp(sc), F.normalize(rot), torch.sigmoid(op), sh

    rows = {
        "state_at_time": lambda t: infer.state_at_time(state, t),
        "  hexplane_points": lambda t: _C.hexplane_points(xyz, tcol(t), state.aabb),
        "  hexplane_forward (packed)": lambda t: _C.hexplane_forward_packed(
            pts0, state.packed, state.plane_f, state.plane_w, state.plane_h, state.order),
        "  deform_infer": lambda t: _C.deform_infer(feat0, state.wf, state.bf, state.w1, state.b1, state.w2, state.b2,
                                                    state.roles, xyz, state.scaling, state.rotation, state.opacity,
                                                    state.f_dc, state.f_rest, True),
        "parent formulation": parent,
    }
    by_cam = {c.time: c for c in cams}
    rows["render_view"] = lambda t: infer.render_view(by_cam[t], state, bg)
    for fn in rows.values():  # warm-up: every shape, both formulations
        for t in times[:5]:
            fn(t)
    torch.cuda.synchronize()
    a, b = infer.state_at_time(state, 0.37), parent(0.37)
    diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
    res = {k: [] for k in rows}
    for _ in range(ROUNDS):  # the formulations alternate within every round
        for k, fn in rows.items():
            res[k].append(per_frame_us(fn, times))
    print(f"infer_time: P = {P}, {W}x{H}, dynerf (F = 32, W = 128, heads 3/3/4/1/48), {FRAMES} timestamps, "
          f"{ROUNDS} alternating rounds; us per frame: median [min .. max]")
    for k, v in res.items():
        print(f"{k:28s} {statistics.median(v):9.1f}  [{min(v):9.1f} .. {max(v):9.1f}]", flush=True)
    print(f"largest |state_at_time - parent formulation| over the five outputs at t = 0.37: {diff:.3e}")
    fps = [infer.render_set(state, cams, bg, keep_images=False)[1] for _ in range(3)]
    print(f"render_set over {FRAMES} cameras: {statistics.median(fps):.1f} FPS  [{min(fps):.1f} .. {max(fps):.1f}]")


if __name__ == "__main__":
    main()
