"""GPU parity of the train-step kernels against the reference's PyTorch
formulations, which are the oracle for these rows (each is a restatement of reference Python,
cited in gs4d_train/): the fused L1 loss vs utils/loss_utils.l1_loss + autograd, the densification
statistics vs train.py:346-349 / gaussian_model.py:521-523, FusedAdam vs torch.optim.Adam as the
reference configures it, the fused HexPlane field vs scene/hexplane.py's F.grid_sample graph, and a
whole train step fused vs unfused.  Tolerances are stated per test.
The deformation module's dispatch between these kernels, route by route against the fp64 unfused graph:
tests/test_deformation_routes_gpu.py (scenes: deformation_route_scenes.py, CPU preconditions: test_deformation_routes_boundary.py)."""

import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", [(101, 77), (100, 76)])  # n % 4 != 0: scalar kernels; n % 4 == 0: float4 / char4
def test_l1_loss_matches_torch(H, W):
    from gs4d_train.kernels import l1_loss
    from gs4d_train.losses import l1_loss_torch
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(2, 3, H, W, device="cuda", generator=g).requires_grad_(True)
    y = torch.rand(2, 3, H, W, device="cuda", generator=g)
    y[0, 0, 0, :5] = x.detach()[0, 0, 0, :5]  # exact ties: subgradient 0
    x2 = x.detach().clone().requires_grad_(True)
    l_f = l1_loss(x, y)
    l_t = l1_loss_torch(x2, y)
    (3.0 * l_f).backward()
    (3.0 * l_t).backward()
    assert abs(l_f.item() - l_t.item()) <= 1e-6 * abs(l_t.item())
    torch.testing.assert_close(x.grad, x2.grad, rtol=0, atol=0)  # sign * (g / N): bitwise


@pytest.mark.parametrize("dloss", [1.0, 0.37])
def test_l1_loss_grad_one_pass_matches_two_pass(dloss):
    """gs4d_l1_loss_grad (value and gradient in one launch, the bench step's form) is bitwise the two-pass
    l1_forward + l1_backward for the same upstream gradient, and the value is torch's L1 to 1e-6."""
    from gs4d_train import _C
    torch.manual_seed(7)
    x = torch.rand(3, 101, 76, device="cuda")
    y = torch.rand(3, 101, 76, device="cuda")
    y[0, 0, :8] = x[0, 0, :8]  # exact ties: sign 0
    loss, grad = _C.l1_loss_grad(x, y, dloss)
    for _ in range(3):  # one launch: its last workgroup sums the partials and re-zeroes the completion counter
        again = _C.l1_loss_grad(x, y, dloss)
        assert torch.equal(again[0], loss) and torch.equal(again[1], grad)
    big = torch.rand(3, 1014, 1352, device="cuda")  # the bench image: ~2000 workgroups
    lb, gb = _C.l1_loss_grad(big, y.new_zeros(big.shape), 1.0)
    lb2, sb = _C.l1_forward(big, torch.zeros_like(big))
    assert torch.equal(lb, lb2) and torch.equal(gb, _C.l1_backward(sb, torch.ones(1, device="cuda")))
    loss2, sgn = _C.l1_forward(x, y)
    grad2 = _C.l1_backward(sgn, torch.full((1,), dloss, device="cuda"))
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert abs(float(loss) - float((x - y).abs().mean())) <= 1e-6
    assert float(grad[0, 0, :8].abs().max()) == 0.0


def test_densify_stats_match_reference():
    from gs4d_train.kernels import densify_stats
    P = 10007
    g = torch.Generator(device="cuda").manual_seed(1)
    vs = torch.randn(P, 3, device="cuda", generator=g)
    vis = torch.rand(P, device="cuda", generator=g) > 0.3
    radii = torch.randint(0, 40, (P,), device="cuda", generator=g, dtype=torch.int32)
    acc, den, mr = torch.rand(P, 1, device="cuda"), torch.randint(0, 5, (P, 1), device="cuda").float(), \
        torch.rand(P, device="cuda") * 30
    acc2, den2, mr2 = acc.clone(), den.clone(), mr.clone()
    densify_stats(vs, vis, radii, acc, den, mr)
    mr2[vis] = torch.max(mr2[vis], radii[vis])
    acc2[vis] += torch.norm(vs[vis, :2], dim=-1, keepdim=True)
    den2[vis] += 1
    torch.testing.assert_close(den, den2, rtol=0, atol=0)
    torch.testing.assert_close(mr, mr2, rtol=0, atol=0)
    torch.testing.assert_close(acc, acc2, rtol=2e-7, atol=0)


def test_fused_adam_matches_torch_adam():
    from gs4d_train.kernels import FusedAdam
    torch.manual_seed(2)
    shapes = [(1000, 3), (777, 1, 3), (777, 15, 3), (128, 128), (128,), (1, 16, 150, 64), (5,)]
    ps = [torch.randn(s, device="cuda") for s in shapes]
    qa = [torch.nn.Parameter(p.clone()) for p in ps]
    qb = [torch.nn.Parameter(p.clone()) for p in ps]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 1.6e-4, 1.6e-4, 1.6e-3, 0.05]
    ga = [{"params": [q], "lr": lr} for q, lr in zip(qa, lrs)]
    gb = [{"params": [q], "lr": lr} for q, lr in zip(qb, lrs)]
    oa = torch.optim.Adam(ga, lr=0.0, eps=1e-15)
    ob = FusedAdam(gb, lr=0.0, eps=1e-15)
    for it in range(6):
        grads = [torch.randn(s, device="cuda") * (10.0 ** (it % 3 - 1)) for s in shapes]
        for q, gr in zip(qa, grads):
            q.grad = gr.clone()
        for q, gr in zip(qb, grads):
            q.grad = gr.clone()
        oa.step()
        ob.step()
    for a, b in zip(qa, qb):
        torch.testing.assert_close(b, a, rtol=2e-6, atol=1e-7)
        sa, sb = oa.state[a], ob.state[b]
        torch.testing.assert_close(sb["exp_avg"], sa["exp_avg"], rtol=1e-6, atol=1e-9)
        torch.testing.assert_close(sb["exp_avg_sq"], sa["exp_avg_sq"], rtol=1e-6, atol=1e-12)
        assert float(sb["step"]) == float(sa["step"])


def test_fused_adam_vector_and_scalar_paths_agree_bitwise():
    """adam_kernel loads 16-byte aligned tensors as float4 and others element by element: the same float
    sequence either way, so a parameter stored 4 bytes off alignment gets bitwise the same update."""
    from gs4d_train.kernels import FusedAdam
    torch.manual_seed(4)
    n = 10_003
    p0 = torch.randn(n, device="cuda")
    store = torch.zeros(n + 1, device="cuda")
    store[1:] = p0
    qa = torch.nn.Parameter(p0.clone())               # aligned: the float4 path (+ 3 tail elements)
    qb = torch.nn.Parameter(store[1:])                # 4 bytes past alignment: the scalar path
    assert qa.data_ptr() % 16 == 0 and qb.data_ptr() % 16 == 4
    oa = FusedAdam([{"params": [qa], "lr": 1e-3}], lr=1e-3, eps=1e-15)
    ob = FusedAdam([{"params": [qb], "lr": 1e-3}], lr=1e-3, eps=1e-15)
    for it in range(3):
        g = torch.randn(n, device="cuda")
        qa.grad, qb.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    assert torch.equal(qa, qb)
    assert torch.equal(oa.state[qa]["exp_avg"], ob.state[qb]["exp_avg"])
    assert torch.equal(oa.state[qa]["exp_avg_sq"], ob.state[qb]["exp_avg_sq"])


def _field(F=16, reso=(64, 64, 64, 150), multires=(1, 2)):
    from gs4d_train.deformation import HexPlaneField
    torch.manual_seed(3)
    f = HexPlaneField(1.6, {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": F,
                            "resolution": list(reso)}, list(multires)).cuda()
    with torch.no_grad():
        for level in f.grids:  # random time planes too (init is all-ones)
            for p in level:
                p.uniform_(0.1, 1.2)
    return f


def test_hexplane_point_order_is_only_locality():
    """_C.hexplane_forward with a caller-kept point order (kernels._HexPlane keeps one across calls): any
    permutation gives bit-identical features (each point is evaluated alone) and the same gradients to
    fp32 summation order (1e-5 of each tensor's max); a stale order of the wrong length is recomputed."""
    from gs4d_train import _C
    f = _field(16)
    planes = [p.detach() for l in f.grids for p in l]
    N = 30000
    g = torch.Generator(device="cuda").manual_seed(7)
    pts = torch.rand(N, 4, device="cuda", generator=g) * 2 - 1
    feat0, packed0, order0 = _C.hexplane_forward(pts, planes)
    perm = torch.randperm(N, device="cuda", generator=g).to(torch.int32)
    feat1, packed1, order1 = _C.hexplane_forward(pts, planes, perm)
    assert order1.data_ptr() == perm.data_ptr()
    assert torch.equal(feat0, feat1)
    dfeat = torch.randn_like(feat0)
    d0, g0 = _C.hexplane_backward(pts, planes, packed0, dfeat, order0)
    d1, g1 = _C.hexplane_backward(pts, planes, packed1, dfeat, order1)
    torch.testing.assert_close(d1, d0, rtol=0, atol=1e-5 * d0.abs().max().item())
    for a, b in zip(g0, g1):
        torch.testing.assert_close(b, a, rtol=0, atol=1e-5 * max(a.abs().max().item(), 1e-30))
    _, _, order2 = _C.hexplane_forward(pts[:100], planes, perm)  # wrong length: a fresh order
    assert order2.numel() == 100 and order2.data_ptr() != perm.data_ptr()


@pytest.mark.parametrize("F,N", [(4, 20000), (8, 20000), (16, 20000), (32, 20000), (16, 100_000)])
def test_hexplane_fused_matches_grid_sample(F, N):
    """The fused field against interpolate_ms_features' grid_sample graph: F = 4..32 (the gather's lane
    split between tap slots and feature groups), points spread over the field and border-clipped."""
    from gs4d_train.deformation import interpolate_ms_features
    from gs4d_train.kernels import hexplane
    f = _field(F)
    g = torch.Generator(device="cuda").manual_seed(4)
    pts = torch.rand(N, 4, device="cuda", generator=g) * 2.4 - 1.2  # incl. border-clamped coordinates
    pts[:100, 0] = 1.0      # exactly on the border (clipped: zero coordinate gradient)
    pts[100:200, 3] = -1.0
    pa = pts.clone().requires_grad_(True)
    pb = pts.clone().requires_grad_(True)
    fa = interpolate_ms_features(pa, f.grids)
    fb = hexplane(pb, [list(l) for l in f.grids])
    torch.testing.assert_close(fb, fa, rtol=1e-5, atol=1e-6)
    up = torch.randn_like(fa)
    ga = torch.autograd.grad(fa, [pa] + [p for l in f.grids for p in l], up)
    gb = torch.autograd.grad(fb, [pb] + [p for l in f.grids for p in l], up)
    torch.testing.assert_close(gb[0], ga[0], rtol=1e-4, atol=1e-4 * ga[0].abs().max().item())
    for a, b in zip(ga[1:], gb[1:]):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5 * max(a.abs().max().item(), 1e-6))


@pytest.mark.parametrize("one_time", [False, True])
def test_hexplane_backward_deterministic(one_time):
    """The backward is deterministic by construction: every term is rounded once to 64-bit fixed point and
    summed exactly (LDS windows, integer atomics), so two backward passes -- and a pass over the same points
    in another visiting order -- give bitwise-equal plane gradients, which match grid_sample's graph.
    one_time: every point at one timestamp, as in a training step (a single view), so the time planes'
    cells collect the taps of thousands of points."""
    from gs4d_train import _C
    from gs4d_train.deformation import interpolate_ms_features
    f = _field(16)
    planes = [p.detach() for l in f.grids for p in l]
    g = torch.Generator(device="cuda").manual_seed(11)
    pts = torch.rand(100_000, 4, device="cuda", generator=g) * 2 - 1
    if one_time:
        pts[:, 3] = 0.3137
    feat, packed, order = _C.hexplane_forward(pts, planes)
    dfeat = torch.randn_like(feat)
    d0, g0 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    d1, g1 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    assert torch.equal(d0, d1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # another visiting order (other workgroups, other boxes, other window passes): the same bits
    perm = torch.randperm(pts.shape[0], device="cuda", generator=g).to(torch.int32)
    _, g2 = _C.hexplane_backward(pts, planes, packed, dfeat, perm)
    for a, b in zip(g0, g2):
        assert torch.equal(a, b)
    pa = pts.clone().requires_grad_(True)
    fa = interpolate_ms_features(pa, f.grids)
    ga = torch.autograd.grad(fa, [pa] + [p for l in f.grids for p in l], dfeat)
    torch.testing.assert_close(d0, ga[0], rtol=1e-4, atol=1e-4 * ga[0].abs().max().item())
    for a, b in zip(ga[1:], g0):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5 * max(a.abs().max().item(), 1e-6))


def test_hexplane_backward_nonfinite_and_scales():
    """Fixed-point edge cases: a NaN in dfeat makes the plane gradients NaN (as a float sum would)
    instead of a finite garbage integer; an all-zero dfeat gives exact zeros; gradients a trillion times
    smaller or larger than O(1) keep their relative accuracy (the scale follows the planes' and dfeat's
    magnitudes, per plane)."""
    from gs4d_train import _C
    from gs4d_train.deformation import interpolate_ms_features
    f = _field(16)
    planes = [p.detach() for l in f.grids for p in l]
    g = torch.Generator(device="cuda").manual_seed(12)
    pts = torch.rand(20_000, 4, device="cuda", generator=g) * 2 - 1
    feat, packed, order = _C.hexplane_forward(pts, planes)
    dfeat = torch.randn_like(feat)
    bad = dfeat.clone()
    bad[123, 5] = float("nan")
    _, gn = _C.hexplane_backward(pts, planes, packed, bad, order)
    assert all(bool(torch.isnan(x).all()) for x in gn)
    _, gz = _C.hexplane_backward(pts, planes, packed, torch.zeros_like(dfeat), order)
    assert all(not bool(x.any()) for x in gz)
    pa = pts.clone().requires_grad_(True)
    fa = interpolate_ms_features(pa, f.grids)
    for mag in (1e-12, 1e12):
        ga = torch.autograd.grad(fa, [p for l in f.grids for p in l], dfeat * mag, retain_graph=True)
        _, gm = _C.hexplane_backward(pts, planes, packed, dfeat * mag, order)
        for a, b in zip(ga, gm):
            torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5 * a.abs().max().item())


def test_heads_pack_any_active_subset():
    """The heads' first-layer weights are packed back to back for the ACTIVE heads only: a
    non-contiguous subset of the five (no_do=True, no_dshs=False: pos, scales, rotations, shs) stacks as one view
    without a copy, and a second call reuses the packing (no re-pack: the parameters' storage stays put)."""
    from gs4d_train import config
    from gs4d_train.deformation import DeformNetwork
    hyper, _ = config.dynerf()
    hyper.no_do, hyper.no_dshs = True, False
    net = DeformNetwork(hyper).cuda().deformation_net
    heads = [getattr(net, n) for n in ("pos_deform", "scales_deform", "rotations_deform", "shs_deform")]
    w1, b1 = net._first_layers(heads)
    assert w1.shape == (4 * net.W, net.W) and w1.data_ptr() == heads[0][1].weight.data_ptr()
    ptrs = [h[1].weight.data_ptr() for h in heads]
    w1b, _ = net._first_layers(heads)
    assert w1b.data_ptr() == w1.data_ptr() and ptrs == [h[1].weight.data_ptr() for h in heads]
    assert torch.equal(w1b, torch.cat([h[1].weight for h in heads], 0))


def test_row_surgery_hip_matches_torch_bitwise():
    """Densify, prune and reset_opacity on the GPU: the one-launch row plans (gs4d_rows_assemble, fused=True)
    against the same plans as torch index ops (fused=False) from the same state and RNG seed -- every
    parameter, Adam moment, statistic and the deformation table bitwise equal, after a real train step made the
    state (k-NN-initialised cloud, 20k Gaussians)."""
    from gs4d_train import config, surgery
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    hyper, opt = config.dynerf()
    opt.iterations = 0
    pts, cols = make_point_cloud(20000, seed=5)
    views = make_training_views(1, 320, 240, seed=6)
    bg = torch.ones(3, device="cuda")
    torch.manual_seed(7)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(pts, cols, 1.0)
    g.training_setup(opt)
    g.active_sh_degree = 3
    train_step(g, views, opt, hyper, 3001, bg)
    gen = torch.Generator(device="cuda").manual_seed(3)
    P = g._xyz.shape[0]
    with torch.no_grad():  # opacities spread around the prune threshold below
        g._opacity.copy_(torch.randn(P, 1, device="cuda", generator=gen))
    # every per-Gaussian parameter gets Adam moments (one more optimizer step with random gradients)
    for name, attr in surgery.PARAMS.items():
        p = getattr(g, attr)
        p.grad = torch.randn(p.shape, device="cuda", generator=gen)
    g.optimizer.step()
    g.xyz_gradient_accum = torch.rand(P, 1, device="cuda", generator=gen) * 4e-4
    g.denom = torch.ones(P, 1, device="cuda")
    g._deformation_table = torch.rand(P, device="cuda", generator=gen) > 0.2

    def state(m):
        out = [m._deformation_table.clone()] + [getattr(m, n).clone() for n in surgery.STATS]
        for name, attr in surgery.PARAMS.items():
            p = getattr(m, attr)
            st = m.optimizer.state.get(p, {})
            out += [p.detach().clone()] + [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
        return out

    runs = []
    for fused in (True, False):
        m = copy.deepcopy(g)
        m.fused = fused
        torch.manual_seed(11)
        m.densify(2e-4, 0.005, 0.5, None)
        grown = state(m)
        m.prune(2e-4, 0.4, 0.5, 20)
        pruned = state(m)
        assert 0 < m._xyz.shape[0] < grown[5].shape[0]
        m.reset_opacity()
        runs.append((grown, pruned, state(m), m._xyz.shape[0]))
    (a1, a2, a3, na), (b1, b2, b3, nb) = runs
    assert na == nb and na != P
    assert len(a1) == len(b1) == len(a2) == len(b2) == len(a3) == len(b3) == 5 + 3 * 6
    for x, y in zip(a1 + a2 + a3, b1 + b2 + b3):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("heavy", [False, True])
def test_hexplane_backward_small_cells_heavy_tailed(heavy):
    """The fixed-point plane gradients keep float-level accuracy in small cells (the scale is fitted
    to a global bound, so resolution is absolute).  Since round 6 the bound is sum_i max_f |dfeat_i| (an exponent
    histogram of the points' gradients) times the other planes' maxima, instead of N max|dfeat|.  Against float64
    grid_sample, beside the float32 grid_sample graph (the reference's own arithmetic): in every magnitude band of
    cells (relative to the plane's largest: >= 1e-3, 1e-5, 1e-7, 1e-9) the fused per-cell relative error is within
    1.5x the float32 graph's (max and median, + 1e-6 / 1e-7), with randn dfeat and with 1 % of the points'
    gradients scaled by 1e4 (heavy-tailed).  Measured (profiles/r06/hexplane_heavy_tail.log): equal to the
    float32 graph's to two digits in every band."""
    from gs4d_train import _C
    from gs4d_train.deformation import interpolate_ms_features
    f = _field(16)
    planes = [p.detach() for l in f.grids for p in l]
    g = torch.Generator(device="cuda").manual_seed(21)
    N = 50_000
    pts = torch.rand(N, 4, device="cuda", generator=g) * 2 - 1
    feat, packed, order = _C.hexplane_forward(pts, planes)
    dfeat = torch.randn(feat.shape, device="cuda", generator=g)
    if heavy:
        dfeat[torch.randperm(N, device="cuda", generator=g)[: N // 100]] *= 1e4
    _, gf = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    p64 = [p.double().requires_grad_(True) for p in planes]
    g64 = torch.autograd.grad(interpolate_ms_features(pts.double(), [p64[:6], p64[6:]]), p64, dfeat.double())
    g32 = torch.autograd.grad(interpolate_ms_features(pts, [list(l) for l in f.grids]),
                              [p for l in f.grids for p in l], dfeat)
    checked = 0
    for a, b, r in zip(gf, g32, g64):
        m = float(r.abs().max())
        for lo, hi in ((1e-3, 1.01), (1e-5, 1e-3), (1e-7, 1e-5), (1e-9, 1e-7)):
            sel = (r.abs() >= lo * m) & (r.abs() < hi * m)
            if int(sel.sum()) < 20:
                continue
            ea = ((a.double() - r).abs() / r.abs())[sel]
            eb = ((b.double() - r).abs() / r.abs())[sel]
            assert float(ea.max()) <= 1.5 * float(eb.max()) + 1e-6, (lo, float(ea.max()), float(eb.max()))
            assert float(ea.median()) <= 1.5 * float(eb.median()) + 1e-7, (lo, float(ea.median()), float(eb.median()))
            checked += 1
    assert checked >= 30


def test_hexplane_backward_fallback_repeatable():
    """Planes whose anchor box is too large for the LDS window take the direct-atomic fallback; with per-point
    times on a 150-cell time axis every time plane of both levels does, including the last plane (z, t) of
    level 0 followed by level 1 (a missing barrier there let the next level overwrite the points'
    plane gradients while slow waves still read them).  Eight backward passes: bitwise equal."""
    from gs4d_train import _C
    f = _field(16)
    planes = [p.detach() for l in f.grids for p in l]
    g = torch.Generator(device="cuda").manual_seed(31)
    pts = torch.rand(100_000, 4, device="cuda", generator=g) * 2 - 1
    feat, packed, order = _C.hexplane_forward(pts, planes)
    dfeat = torch.randn(feat.shape, device="cuda", generator=g)
    d0, g0 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    for _ in range(7):
        d1, g1 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
        assert torch.equal(d0, d1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


_TRAIN_PROCESS = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
from gs4d_train import config
from gs4d_train.gaussians import GaussianModel
from gs4d_train.synthetic import make_point_cloud, make_training_views
from gs4d_train.train import train_step
hyper, opt = config.dynerf()
opt.iterations = 0
pts, cols = make_point_cloud(20000, seed=5)
views = make_training_views(2, 320, 240, seed=6)
bg = torch.ones(3, device="cuda")
torch.manual_seed(7)
g = GaussianModel(3, hyper, fused=True)
g.create_from_pcd(pts, cols, 1.0)
g._deformation.deformation_net.grid.fused = True
g._deformation.deformation_net.fused_heads = True
g.training_setup(opt)
g.active_sh_degree = 3
for it in range(3001, 3006):
    train_step(g, views[(it % 2):(it % 2) + 1], opt, hyper, it, bg)
torch.cuda.synchronize()
h = hashlib.sha256()
for t in [p for grp in g.optimizer.param_groups for p in grp["params"]]:
    h.update(t.detach().cpu().numpy().tobytes())
print(h.hexdigest())
"""


def test_train_steps_bitwise_across_processes():
    """Five fused fine-stage train steps (DyNeRF heads: the f32-MFMA GEMMs, the fixed-point HexPlane backward,
    the rasterizer, Adam) in two separate processes end with bitwise-equal parameters: a seed's training run is
    one fixed trajectory (round 5's timing-tuned GEMM kernels could differ between processes)."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4dgaussians-fast-train_amd")
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", _TRAIN_PROCESS, pkg], capture_output=True, text=True, timeout=55)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1] and len(digests[0]) == 64, digests


def test_train_step_deterministic():
    """Two fused fine-stage train steps from the same state give bitwise-equal gradients of every
    parameter and bitwise-equal statistics, by default (no opt-in: the HexPlane field's backward sums exact
    fixed-point terms and every other kernel of the step reduces in a fixed order)."""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    hyper, opt = config.dynerf()
    opt.iterations = 0
    pts, cols = make_point_cloud(20000, seed=5)
    views = make_training_views(2, 320, 240, seed=6)
    bg = torch.ones(3, device="cuda")
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        g = GaussianModel(3, hyper, fused=True)
        g.create_from_pcd(pts, cols, 1.0)
        g._deformation.deformation_net.grid.fused = True
        g._deformation.deformation_net.fused_heads = True
        g.training_setup(opt)
        g.active_sh_degree = 3
        loss = float(train_step(g, views, opt, hyper, 3001, bg))
        grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            grads[name] = getattr(g, name).grad.detach().clone()
        runs.append((loss, grads, g.xyz_gradient_accum.clone()))
    (la, ga, aa), (lb, gb, ab) = runs
    assert la == lb
    assert any("grid" in k for k in ga)
    differ = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not differ, differ
    assert torch.equal(aa, ab)


def test_hexplane_regulation_fused_matches_torch():
    """kernels.hexplane_regulation vs the reference's compute_regulation graph (scene/regulation.py:22-28,
    scene/gaussian_model.py:538-577): loss to 1e-5 relative (fp64 partials vs torch's fp32 means),
    every plane gradient to 1e-5 of its tensor's maximum; levels of DyNeRF's shape, random values
    (time planes around their init of 1, with exact ones for the |1 - t| subgradient)."""
    from types import SimpleNamespace

    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.kernels import hexplane_regulation
    torch.manual_seed(3)
    F = 16
    grids_t, grids_f = [], []
    for reso in ([64, 64, 64, 150], [128, 128, 128, 150]):
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        lvl = []
        for c0, c1 in pairs:
            t = torch.rand(1, F, reso[c1], reso[c0], device="cuda")
            if c1 == 3:
                t = 1.0 + 0.05 * (t - 0.5)
                t.view(-1)[:100] = 1.0
            lvl.append(t)
        grids_t.append([t.clone().requires_grad_(True) for t in lvl])
        grids_f.append([t.clone().requires_grad_(True) for t in lvl])
    w = (1.0, 1e-4, 2e-4)  # time_smoothness_weight, l1_time_planes, plane_tv_weight (dynerf default)
    g = GaussianModel.__new__(GaussianModel)
    g.fused = False
    g._deformation = SimpleNamespace(deformation_net=SimpleNamespace(grid=SimpleNamespace(grids=grids_t)))
    lt = g.compute_regulation(*w)
    lf = hexplane_regulation(grids_f, *w)
    (2.5 * lt).backward()
    (2.5 * lf).backward()
    assert abs(lf.item() - lt.item()) <= 1e-5 * abs(lt.item())
    for a, b in zip([p for l in grids_f for p in l], [p for l in grids_t for p in l]):
        scale = max(float(b.grad.abs().max()), 1e-30)
        assert float((a.grad - b.grad).abs().max()) <= 1e-5 * scale
    # the train step's form: value and gradient from one pass (accumulate_grad with_value) -- the value bitwise
    # hexplane_regulation_value's, the gradient bitwise the accumulate-only pass's
    from gs4d_train.kernels import hexplane_regulation_accumulate_grad, hexplane_regulation_value
    ga = [[p.detach().clone().requires_grad_(True) for p in l] for l in grids_f]
    gb = [[p.detach().clone().requires_grad_(True) for p in l] for l in grids_f]
    v = hexplane_regulation_accumulate_grad(ga, *w, scale=2.5, with_value=True)
    assert hexplane_regulation_accumulate_grad(gb, *w, scale=2.5) is None
    assert torch.equal(v, hexplane_regulation_value(ga, *w))
    for a, b in zip([p for l in ga for p in l], [p for l in gb for p in l]):
        assert torch.equal(a.grad, b.grad)
    # with a base (the train step's L1 value): base + value from the same launch, bitwise torch's fp32 add; the
    # last-workgroup total re-arms its ticket, so repeated calls agree
    base = torch.full((), 0.0123456789, device="cuda")
    for _ in range(3):
        gc = [[p.detach().clone().requires_grad_(True) for p in l] for l in grids_f]
        vb = hexplane_regulation_accumulate_grad(gc, *w, scale=2.5, with_value=True, base=base)
        assert torch.equal(vb, base + v)
        for a, b in zip([p for l in gc for p in l], [p for l in gb for p in l]):
            assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1]), (777, 64, [2, 5, 8]), (3000, 256, [16, 7]),
                                     (50_001, 128, [48]), (1, 128, [1, 48]), (0, 128, [3])])
def test_linear_dw_matches_fp64(P, W, ns):
    """gs4d_linear_dw (the narrow deformation heads' weight/bias gradients, dW = dy^T x, db = dy.sum(0))
    vs fp64 torch: to 1e-5 of each result's largest |term sum| (fp32 partial sums over ~1e5 rows); x a
    column block of a wider matrix as in the heads block; ragged P (not a multiple of the row blocks),
    P = 1 and P = 0."""
    from gs4d_train import _C
    torch.manual_seed(P + W)
    a = torch.relu(torch.randn(P, len(ns) * W + 5, device="cuda"))
    dys = [torch.randn(P, n, device="cuda") for n in ns]
    xs = [a[:, 5 + i * W:5 + (i + 1) * W] for i in range(len(ns))]
    out = _C.linear_dw(dys, xs)
    for i, (d, x) in enumerate(zip(dys, xs)):
        rw, rb = d.double().t() @ x.double(), d.double().sum(0)
        sw = (d.double().abs().t() @ x.double().abs()).max().clamp_min(1e-30)
        sb = d.double().abs().sum(0).max().clamp_min(1e-30)
        assert out[2 * i].shape == (ns[i], W) and out[2 * i + 1].shape == (ns[i],)
        assert float((out[2 * i].double() - rw).abs().max() / sw) <= 1e-5
        assert float((out[2 * i + 1].double() - rb).abs().max() / sb) <= 1e-5


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1, 48]), (777, 64, [2, 16, 5]), (1, 128, [1, 48]),
                                     (0, 128, [3, 4]), (1001, 64, [48, 3, 48]), (300, 256, [16, 1])])
def test_heads_backward_matches_fp64(P, W, ns):
    """gs4d_heads_backward (the heads block's second layers + ReLU mask + first-layer bias gradient in one
    pass) vs the same products in fp64 torch: da to 1e-5 of its row's |terms| sum, the reductions to 1e-5 of
    their largest |term| sum; the mask exact (a > 0, zeros kept); ragged P, P = 1 and P = 0."""
    from gs4d_train import _C
    torch.manual_seed(P + W)
    k = len(ns)
    a = torch.relu(torch.randn(P, k * W, device="cuda"))
    gs = [torch.randn(P, n, device="cuda") for n in ns]
    w2 = [torch.randn(n, W, device="cuda") for n in ns]
    out = _C.heads_backward(a, gs, w2)
    da, db1 = out[0], out[1]
    ad = a.double()
    ref = torch.cat([g.double() @ w.double() for g, w in zip(gs, w2)], 1) * (ad > 0)
    scale = torch.cat([g.double().abs() @ w.double().abs() for g, w in zip(gs, w2)], 1)
    assert da.shape == a.shape and db1.shape == (k * W,)
    assert bool(((da == 0) == ((a <= 0) | (ref == 0))).all()) or P == 0
    assert float(((da.double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0 if P else True
    s1 = (ref.abs().sum(0).max() if P else torch.tensor(1.0)).clamp_min(1e-30)
    assert float((db1.double() - ref.sum(0)).abs().max() / s1) <= 1e-5
    for i, (g, w) in enumerate(zip(gs, w2)):
        x = ad[:, i * W:(i + 1) * W]
        rw, rb = g.double().t() @ x, g.double().sum(0)
        sw = (g.double().abs().t() @ x.abs()).max().clamp_min(1e-30)
        sb = g.double().abs().sum(0).max().clamp_min(1e-30)
        assert float((out[2 + 2 * i].double() - rw).abs().max() / sw) <= 1e-5
        assert float((out[3 + 2 * i].double() - rb).abs().max() / sb) <= 1e-5


def test_heads_backward_wide_head_needs_w_64_or_128():
    """The 48-wide head has MFMA kernels for W in {64, 128} only: gs4d_heads_backward rejects it at W = 256
    (the argument check that keeps a wide head from ever reaching a narrow kernel) and serves it at W = 128
    with results of the documented shapes (da, db1, dW2, db2)."""
    from gs4d_train import _C
    torch.manual_seed(48)
    P, n = 8, 48
    for W, ok in ((256, False), (128, True)):
        a = torch.relu(torch.randn(P, W, device="cuda"))
        gs, w2 = [torch.randn(P, n, device="cuda")], [torch.randn(n, W, device="cuda")]
        if not ok:
            with pytest.raises(RuntimeError):
                _C.heads_backward(a, gs, w2)
            continue
        out = _C.heads_backward(a, gs, w2)
        assert [tuple(t.shape) for t in out] == [(P, W), (W,), (n, W), (n,)]
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in out)


@pytest.mark.parametrize("P,N,K,col0", [(100_000, 640, 128, 0), (100_003, 640, 128, 0), (2048, 640, 128, 0),
                                         (5000, 192, 64, 0), (3001, 256, 256, 0), (7777, 128, 128, 5)])
def test_mlp_gemms_match_fp64(P, N, K, col0):
    """The deformation MLP's GPU GEMMs on rocBLAS (deformation._splitk_dw: split-K chunk partials + their
    remainder + gs4d_sum_slices; deformation._mm_dx: dy @ W) vs fp64 torch, to 1e-5 of each result's largest
    |term| sum; P with a chunk that divides it (100k: 2000 rows, _chunk_rows) and P with a remainder, x a column
    block of a wider matrix (col0 > 0),
    W 64/128/256.  The tuned kernel of each shape class is the one that runs (gemm_tuned), rocBLAS's own
    pick (tune=False) computes the same product, and gs4d_sum_slices' scalar form."""
    from gs4d_train import _C, deformation as D
    torch.manual_seed(P + N)
    dy = torch.randn(P, N, device="cuda")
    wide = torch.relu(torch.randn(P, col0 + K + 3, device="cuda"))
    x = wide[:, col0:col0 + K]
    dw = D._splitk_dw(dy, x)
    ref = dy.double().t() @ x.double()
    scale = (dy.double().abs().t() @ x.double().abs()).max()
    assert dw.shape == (N, K)
    assert float((dw.double() - ref).abs().max() / scale) <= 1e-5
    w = torch.randn(N, K, device="cuda")
    dx = D._mm_dx(dy, w)
    refx = dy.double() @ w.double()
    assert dx.shape == (P, K)
    assert float(((dx.double() - refx).abs() - 1e-5 * (dy.double().abs() @ w.double().abs())).max()) <= 0
    # the kernel chosen for a shape class (gemm_f32 tune=True) is the one that runs at the train step's shapes:
    # a second call reports the cached choice, and every tuned class has a record (no rejected index)
    o = torch.empty(P, K, device="cuda")
    sol = _C.gemm_f32(w, dy, o, False, False, K, P, N, K, N, K, 1, 0, 0, 0, True)
    tuned = {k: v for k, v, *_ in _C.gemm_tuned()}
    def bucket(v):  # train_glue.cpp dim_bucket: sizes above 4096 by 1/8-octave classes
        if v <= 4096:
            return v
        step = 1 << (v.bit_length() - 4)
        return -(-v // step) * step
    key = f"f32 nn m={K} n={bucket(P)} k={N} lda={K} ldb={N} ldc={K} batch=1 dev={o.device.index}"
    assert tuned.get(key) == sol, (key, sol, tuned)
    # the tuner compared real kernels: rocBLAS's own pick and at least one more whose product matched (a check
    # that rejects every candidate leaves the library's pick alone, silently)
    cands = {k: c for k, _, _, _, c in _C.gemm_tuned()}
    assert cands[key] >= 2, (key, cands[key])
    assert float(((o.double() - refx).abs() - 1e-5 * (dy.double().abs() @ w.double().abs())).max()) <= 0
    if P >= 4096:
        S = P // 1024
        parts = torch.empty(S, N, K, device="cuda")
        sol_b = _C.gemm_f32(x, dy, parts, False, True, K, N, 1024, x.stride(0), N, K, S, 1024 * x.stride(0),
                            1024 * N, N * K, True)
        tuned = {k: v for k, v, *_ in _C.gemm_tuned()}
        assert any(v == sol_b and f"batch={S} " in k for k, v in tuned.items()), (sol_b, tuned)
    # the library's own kernel (solution 0) computes the same product
    out = torch.empty(P, K, device="cuda")
    assert _C.gemm_f32(w, dy, out, False, False, K, P, N, K, N, K, 1, 0, 0, 0, False) == 0
    assert float(((out.double() - refx).abs() - 1e-5 * (dy.double().abs() @ w.double().abs())).max()) <= 0
    # an operand that does not fit its tensor is refused before any launch
    with pytest.raises(RuntimeError):
        _C.gemm_f32(w, dy, out, False, False, K, P + 1, N, K, N, K, 1, 0, 0, 0, True)
    parts = torch.randn(5, 7, 3, device="cuda")  # n = 21: the scalar form
    assert torch.equal(_C.sum_slices(parts), (((parts[0] + parts[1]) + parts[2]) + parts[3]) + parts[4])


def test_sum_slices_quarter_tree():
    """gs4d_sum_slices with many slices (S >= 16, float4 rows): each quarter of the slices summed in slice order,
    the quarters as (q0 + q1) + (q2 + q3) -- a fixed tree, checked bit for bit (float adds done the same way by
    torch), with a ragged quarter split (S = 37) and a partial last wave (50 float4 outputs)."""
    from gs4d_train import _C
    torch.manual_seed(11)
    S = 37
    parts = torch.randn(S, 50, 4, device="cuda")

    def seq(a, b):
        acc = torch.zeros_like(parts[0])
        for s in range(a, b):
            acc = acc + parts[s]
        return acc

    q = [seq(g * S // 4, (g + 1) * S // 4) for g in range(4)]
    assert torch.equal(_C.sum_slices(parts), (q[0] + q[1]) + (q[2] + q[3]))


def test_hexplane_fused_matches_reference_module():
    """The fused HexPlane kernels (the field's input points, forward and backward in HIP) against vectors made
    by RUNNING the reference's scene/hexplane.py (tests/golden/ref_hexplane_vectors.npz; F = 4, two levels,
    points beyond the bounds and times beyond [-1, 1]: border clipping): features to 1e-5 relative, the point
    and plane gradients to 1e-4 of each tensor's maximum (summation order)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_harness_cpu import _ref_hexplane_field
    field, v = _ref_hexplane_field("cuda")
    field.fused = True
    pts = torch.from_numpy(v["pts"]).cuda().requires_grad_(True)
    feat = field(pts, torch.from_numpy(v["times"]).cuda())
    ref = torch.from_numpy(v["feat"]).cuda()
    assert float((feat.detach() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    (feat * torch.from_numpy(v["G"]).cuda()).sum().backward()
    pairs = [(pts.grad, v["gpts"])] + [(pl.grad, v[f"gplane_{li}_{pi}"]) for li, level in enumerate(field.grids)
                                       for pi, pl in enumerate(level)]
    for got, exp in pairs:
        exp = torch.from_numpy(exp).cuda()
        assert float((got - exp).abs().max()) <= 1e-4 * max(float(exp.abs().max()), 1e-30)


def test_hexplane_points_match_reference_graph():
    """gs4d_hexplane_points (normalize_aabb + cat with the time column, scene/hexplane.py:20-21, 166) and its
    backward vs the reference's torch graph: bitwise equal both ways (the same float operations)."""
    from gs4d_train.deformation import normalize_aabb
    from gs4d_train.kernels import hexplane_points
    torch.manual_seed(3)
    N = 10007
    xyz = (torch.randn(N, 3, device="cuda") * 2).requires_grad_(True)
    t = torch.rand(N, 1, device="cuda")
    aabb = torch.tensor([[1.3, 1.7, 2.1], [-1.1, -1.9, -0.7]], device="cuda")
    x2 = xyz.detach().clone().requires_grad_(True)
    ref = torch.cat((normalize_aabb(x2, aabb), t), dim=-1)
    out = hexplane_points(xyz, t, aabb)
    torch.testing.assert_close(out, ref, rtol=0, atol=0)
    g = torch.randn(N, 4, device="cuda")
    ref.backward(g)
    out.backward(g)
    torch.testing.assert_close(xyz.grad, x2.grad, rtol=0, atol=0)


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1, 48]), (777, 64, [2, 16, 5]), (1, 128, [1, 48]),
                                     (0, 128, [3, 4]), (1001, 256, [17, 40]), (40, 128, [33, 64])])
def test_heads_forward_matches_fp64(P, W, ns):
    """gs4d_heads_forward (the heads block's second layers in one MFMA pass over a) vs the same products
    in fp64 torch: every output to 1e-5 of its |terms| sum (+ |bias|); ragged P, P = 1, P = 0, n_i from 1
    to 64 (partial 16-output tiles)."""
    from gs4d_train import _C
    torch.manual_seed(P + W + len(ns))
    k = len(ns)
    a = torch.relu(torch.randn(P, k * W, device="cuda"))
    w2 = [torch.randn(n, W, device="cuda") for n in ns]
    b2 = [torch.randn(n, device="cuda") for n in ns]
    out = _C.heads_forward(a, w2, b2)
    assert len(out) == k
    for i, (w, b) in enumerate(zip(w2, b2)):
        x = a[:, i * W:(i + 1) * W].double()
        ref = x @ w.double().t() + b.double()
        scale = x.abs() @ w.double().abs().t() + b.double().abs()
        assert out[i].shape == (P, ns[i])
        if P:
            assert float(((out[i].double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1, 48]), (777, 64, [2, 16, 5]), (1, 128, [1, 48]),
                                     (0, 128, [3, 4]), (40, 128, [33, 64]), (5000, 64, [3, 3, 4])])
def test_heads_block_forward_matches_fp64(P, W, ns):
    """gs4d_heads_block_forward (both layers of the heads block in one MFMA pass) vs fp64 torch: a =
    relu(h W1^T + b1) to 1e-5 of its |terms| sum, and every head output, formed from the kernel's own a,
    to 1e-5 of its |terms| sum; ragged P, P = 1, P = 0, n_i from 1 to 64."""
    from gs4d_train import _C
    torch.manual_seed(P + 7 * W + len(ns))
    k = len(ns)
    h = torch.relu(torch.randn(P, W, device="cuda"))
    w1 = torch.randn(k * W, W, device="cuda") / W ** 0.5
    b1 = torch.randn(k * W, device="cuda") * 0.1
    w2 = [torch.randn(n, W, device="cuda") / W ** 0.5 for n in ns]
    b2 = [torch.randn(n, device="cuda") for n in ns]
    a, w1t, *out = _C.heads_block_forward(h, w1, b1, w2, b2)
    assert a.shape == (P, k * W) and len(out) == k and w1t.shape == (W, k * W)
    if P == 0:
        return
    assert torch.equal(w1t, w1.t())  # written by the same pass for the backward (gs4d_mlp_dx_f32)
    hd = h.double()
    z = hd @ w1.double().t() + b1.double()
    za = hd.abs() @ w1.double().abs().t() + b1.double().abs()
    assert float(((a.double() - torch.relu(z)).abs() - 1e-5 * za).max().clamp_min(0)) == 0.0
    for i, (w, b) in enumerate(zip(w2, b2)):
        x = a[:, i * W:(i + 1) * W].double()
        ref = x @ w.double().t() + b.double()
        scale = x.abs() @ w.double().abs().t() + b.double().abs()
        assert out[i].shape == (P, ns[i])
        assert float(((out[i].double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0


BF16_ULP = 2.0 ** -8  # one bf16 ulp relative (8 significant bits): a value rounded once lands within it


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1, 48]), (777, 64, [2, 16, 5]), (1, 128, [1, 48]),
                                     (0, 128, [3, 4]), (40, 128, [33, 64]), (5000, 64, [3, 3, 4])])
def test_heads_block_forward_bf16_matches_fp64(P, W, ns):
    """gs4d_heads_block_forward_bf16 (both layers on the bf16 MFMA) vs fp64 torch on the same bf16-rounded
    operands: hb is exactly h rounded to bf16 (round-to-nearest-even, as torch); a = bf16(relu(h W1^T + b1))
    within one bf16 ulp of the fp64 value + 1e-5 of its |terms| sum (fp32 accumulation); every head output,
    formed from the kernel's own bf16 a and bf16 W2, within 1e-5 of its |terms| sum.  Ragged P, P = 1, 0."""
    from gs4d_train import _C
    torch.manual_seed(P + 7 * W + len(ns))
    k = len(ns)
    h = torch.relu(torch.randn(P, W, device="cuda"))
    w1 = torch.randn(k * W, W, device="cuda") / W ** 0.5
    b1 = torch.randn(k * W, device="cuda") * 0.1
    w2 = [torch.randn(n, W, device="cuda") / W ** 0.5 for n in ns]
    b2 = [torch.randn(n, device="cuda") for n in ns]
    a, hb, w1t, *out = _C.heads_block_forward_bf16(h, w1, b1, w2, b2)
    assert a.dtype == hb.dtype == torch.bfloat16 and a.shape == (P, k * W) and hb.shape == (P, W) and len(out) == k
    if P:
        assert torch.equal(w1t, w1.t().to(torch.bfloat16))
    if P == 0:
        return
    bf = torch.bfloat16
    assert torch.equal(hb, h.to(bf))
    # the same block fed h already rounded to bf16 (the train path's _FeatureReLUHB copy): bitwise the same
    hbin = torch.empty((P + 15) // 16 * 16, W, device="cuda", dtype=bf)[:P]
    hbin.copy_(h.to(bf))
    a2, hb2, w1t2, *out2 = _C.heads_block_forward_bf16(h, w1, b1, w2, b2, hb=hbin)
    assert hb2.data_ptr() == hbin.data_ptr() and torch.equal(a2, a) and torch.equal(w1t2, w1t)
    assert all(torch.equal(x, y) for x, y in zip(out2, out))
    hd = h.to(bf).double()
    z = hd @ w1.to(bf).double().t() + b1.double()
    za = hd.abs() @ w1.to(bf).double().abs().t() + b1.double().abs()
    err = (a.double() - torch.relu(z)).abs() - BF16_ULP * torch.relu(z) - 1e-5 * za
    assert float(err.max().clamp_min(0)) == 0.0
    for i, (w, b) in enumerate(zip(w2, b2)):
        x = a[:, i * W:(i + 1) * W].double()
        wd = w.to(bf).double()
        ref = x @ wd.t() + b.double()
        scale = x.abs() @ wd.abs().t() + b.double().abs()
        assert out[i].dtype == torch.float32 and out[i].shape == (P, ns[i])
        assert float(((out[i].double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0


@pytest.mark.parametrize("P,W,ns", [(100_003, 128, [3, 3, 4, 1, 48]), (777, 64, [2, 16, 5]), (1, 128, [1, 48]),
                                     (0, 128, [3, 4]), (1001, 64, [48, 3, 48]), (300, 256, [16, 1])])
def test_heads_backward_bf16_matches_fp64(P, W, ns):
    """gs4d_heads_backward_bf16 (a and da in bf16, everything else fp32) vs fp64 torch on the same bf16 a:
    da within one bf16 ulp + 1e-5 of its row's |terms| sum, the mask exact; db1 (summed before da is
    rounded), dW2 and db2 to 1e-5 of their largest |term| sum.  The 48-wide head at W = 128 runs on the bf16
    MFMA (heads_bwd_wide_bf16_kernel) with g and W2 rounded to bf16 as operands: its references use those
    rounded values (db2 stays the fp32 g's sum).  A wide head the bf16 path has no kernel for (n = 40) is
    refused."""
    from gs4d_train import _C
    torch.manual_seed(P + W + 11 * len(ns))
    k = len(ns)
    bf = torch.bfloat16
    a = torch.relu(torch.randn(P, k * W, device="cuda")).to(bf)
    gs = [torch.randn(P, n, device="cuda") for n in ns]
    w2 = [torch.randn(n, W, device="cuda") for n in ns]
    out = _C.heads_backward(a, gs, w2)
    da, db1 = out[0], out[1]
    assert da.dtype == torch.bfloat16 and da.shape == a.shape and db1.dtype == torch.float32
    ad = a.double()
    wide = [n == 48 and W == 128 for n in ns]
    gq = [g.to(bf).double() if wd else g.double() for g, wd in zip(gs, wide)]
    wq = [w.to(bf).double() if wd else w.double() for w, wd in zip(w2, wide)]
    ref = torch.cat([g @ w for g, w in zip(gq, wq)], 1) * (ad > 0)
    scale = torch.cat([g.abs() @ w.abs() for g, w in zip(gq, wq)], 1)
    if P:
        assert bool(((da == 0) == ((a <= 0) | (ref.abs() < 1e-38))).all())
        err = (da.double() - ref).abs() - BF16_ULP * ref.abs() - 1e-5 * scale
        assert float(err.max().clamp_min(0)) == 0.0
    s1 = (ref.abs().sum(0).max() if P else torch.tensor(1.0)).clamp_min(1e-30)
    assert float((db1.double() - ref.sum(0)).abs().max() / s1) <= 1e-5
    for i, (g, w) in enumerate(zip(gs, w2)):
        x = ad[:, i * W:(i + 1) * W]
        rw, rb = gq[i].t() @ x, g.double().sum(0)
        sw = (gq[i].abs().t() @ x.abs()).max().clamp_min(1e-30)
        sb = g.double().abs().sum(0).max().clamp_min(1e-30)
        assert out[2 + 2 * i].dtype == torch.float32
        assert float((out[2 + 2 * i].double() - rw).abs().max() / sw) <= 1e-5
        assert float((out[3 + 2 * i].double() - rb).abs().max() / sb) <= 1e-5
    if P:
        with pytest.raises(RuntimeError):
            _C.heads_backward(a[:, :W].contiguous(), [torch.randn(P, 40, device="cuda")], [torch.randn(40, W, device="cuda")])


@pytest.mark.parametrize("P,KW,W", [(100_003, 640, 128), (1, 640, 128), (0, 640, 128), (777, 192, 64), (300, 64, 128),
                                     (513, 1024, 128)])
def test_mlp_dx_bf16_matches_fp64(P, KW, W):
    """gs4d_mlp_dx_bf16 (dh = da W1 on the bf16 MFMA from W1^T, the k chunks staged in LDS) vs fp64 products of the
    same bf16 values, to 1e-5 of each element's |terms| sum; ragged P (rows past P read row P - 1 and are not
    stored; partial workgroups), P = 1, 0, one k chunk and sixteen."""
    from gs4d_train import _C
    torch.manual_seed(P + KW + W)
    bf = torch.bfloat16
    da = torch.randn(P, KW, device="cuda").to(bf)
    w1 = (torch.randn(KW, W, device="cuda") / KW ** 0.5).to(bf)
    dh = _C.mlp_dx_bf16(da, w1.t().contiguous())
    assert dh.dtype == torch.float32 and dh.shape == (P, W)
    if P:
        ref = da.double() @ w1.double()
        scale = da.double().abs() @ w1.double().abs()
        assert float(((dh.double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0


@pytest.mark.parametrize("P,KW", [(100_003, 640), (1, 640), (0, 640), (1024, 128), (3000, 256), (33, 640)])
def test_mlp_dw_bf16_matches_fp64(P, KW):
    """gs4d_mlp_dw_bf16 (dW1 = da^T hb on the bf16 MFMA, tiles read back with LDS transpose reads, 1024-row
    chunks summed in order) vs fp64 products of the same bf16 values, to 1e-5 of each element's |terms| sum:
    ragged P (a partial last chunk and a partial 32-row step, staged as zeros), P = 1, 0, one head and five."""
    from gs4d_train import _C
    torch.manual_seed(P + KW)
    bf = torch.bfloat16
    da = torch.randn(P, KW, device="cuda").to(bf)
    hb = torch.relu(torch.randn(P, 128, device="cuda")).to(bf)
    dw = _C.mlp_dw_bf16(da, hb)
    assert dw.dtype == torch.float32 and dw.shape == (KW, 128)
    ref = da.double().t() @ hb.double()
    scale = da.double().abs().t() @ hb.double().abs()
    assert float(((dw.double() - ref).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0


@pytest.mark.parametrize("P,KW,W", [(100_000, 640, 128), (100_003, 640, 128), (1, 640, 128), (0, 640, 128),
                                     (2000, 192, 64), (777, 64, 128), (300, 1024, 64), (65, 128, 128)])
def test_mlp_f32_gemms_match_fp64(P, KW, W):
    """gs4d_mlp_dx_f32 (dh = da W1, from W1^T) and gs4d_mlp_dw_f32 (dW1 = da^T h), the fp32 heads block's two large GEMMs on
    the f32 MFMA, vs fp64 torch: every element to 1e-5 of its |terms| sum (f32 products are exact in f64; the
    bar covers fp32 accumulation over up to 1e5 terms).  Ragged P (partial 64-row groups, a partial last chunk
    and 8-row step: rows past P read row P - 1 and are zeroed / not stored), P = 1 and 0 (dW1 all zeros), one
    k chunk and sixteen, W 64 and 128.  A second call gives the same bits."""
    from gs4d_train import _C
    torch.manual_seed(P + KW + W)
    da = torch.randn(P, KW, device="cuda")
    h = torch.relu(torch.randn(P, W, device="cuda"))
    w1 = torch.randn(KW, W, device="cuda") / KW ** 0.5
    w1t = w1.t().contiguous()
    dh = _C.mlp_dx_f32(da, w1t)
    dw = _C.mlp_dw_f32(da, h)
    assert dh.shape == (P, W) and dw.shape == (KW, W) and dh.dtype == dw.dtype == torch.float32
    refw = da.double().t() @ h.double()
    scw = da.double().abs().t() @ h.double().abs()
    assert float(((dw.double() - refw).abs() - 1e-5 * scw).max().clamp_min(0)) == 0.0
    if P == 0:
        assert bool((dw == 0).all())
        return
    refx = da.double() @ w1.double()
    scx = da.double().abs() @ w1.double().abs()
    assert float(((dh.double() - refx).abs() - 1e-5 * scx).max().clamp_min(0)) == 0.0
    assert torch.equal(_C.mlp_dx_f32(da, w1t), dh) and torch.equal(_C.mlp_dw_f32(da, h), dw)
    with pytest.raises(RuntimeError):  # a W the kernels are not built for is refused, not run
        _C.mlp_dx_f32(da, torch.randn(96, KW, device="cuda"))


_CROSS_PROCESS = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
from gs4d_train import _C
torch.manual_seed(5)
P, KW, W = 100_003, 640, 128
da = torch.randn(P, KW, device="cuda")
h = torch.relu(torch.randn(P, W, device="cuda"))
w1 = torch.randn(KW, W, device="cuda") / KW ** 0.5
out = [_C.mlp_dx_f32(da, w1.t().contiguous()), _C.mlp_dw_f32(da, h)]
torch.cuda.synchronize()
print(hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in out)).hexdigest())
"""


def test_mlp_f32_gemms_bitwise_across_processes():
    """The fp32 heads-block GEMMs give the same bits in two separate processes (the round-5 rocBLAS kernels were
    chosen per process by timing, and differently rounded kernels broke the fused-vs-unfused training pair)."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4dgaussians-fast-train_amd")
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", _CROSS_PROCESS, pkg], capture_output=True, text=True, timeout=55)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1] and len(digests[0]) == 64, digests


@pytest.mark.parametrize("P,N,K", [(100_003, 640, 128), (2048, 640, 128), (5000, 192, 64), (700, 640, 128)])
def test_mlp_gemms_bf16_match_fp64(P, N, K):
    """The bf16 path's GEMMs on rocBLAS (bf16 operands, f32 accumulation and output): the split-K weight
    gradient (deformation._splitk_dw on bf16 da, hb) and the input gradient (deformation._mm_dx on bf16
    W1) vs fp64 products of the same bf16 values, to 1e-5 of each result's |term| sum."""
    from gs4d_train import deformation as D
    torch.manual_seed(P + N + K)
    bf = torch.bfloat16
    dy = torch.randn(P, N, device="cuda").to(bf)
    x = torch.relu(torch.randn(P, K, device="cuda")).to(bf)
    dw = D._splitk_dw(dy, x)
    assert dw.dtype == torch.float32 and dw.shape == (N, K)
    ref = dy.double().t() @ x.double()
    scale = (dy.double().abs().t() @ x.double().abs()).max()
    assert float((dw.double() - ref).abs().max() / scale) <= 1e-5
    w = torch.randn(N, K, device="cuda").to(bf)
    dx = D._mm_dx(dy, w)
    assert dx.dtype == torch.float32 and dx.shape == (P, K)
    refx = dy.double() @ w.double()
    assert float(((dx.double() - refx).abs() - 1e-5 * (dy.double().abs() @ w.double().abs())).max()) <= 0


@pytest.mark.parametrize("P,Fin,Fout", [(100_003, 32, 128), (777, 64, 64), (1, 32, 128), (0, 32, 128),
                                        (333, 32, 64), (16, 64, 64)])
def test_feature_relu_backward_matches_fp64(P, Fin, Fout):
    """gs4d_feature_relu_backward (the first deformation layer's ReLU mask, input gradient, weight and
    bias gradients in one MFMA pass) vs fp64 torch: dx to 1e-5 of its row's |terms| sum, dW / db to
    1e-5 of their largest |term| sum, rows whose h <= 0 contribute exactly nothing; ragged P, P = 1,
    P = 0 (zero gradients); then _FeatureReLU end to end through autograd."""
    from gs4d_train import _C
    from gs4d_train.deformation import _FeatureReLU
    torch.manual_seed(P + Fin)
    x = torch.randn(P, Fin, device="cuda")
    w = torch.randn(Fout, Fin, device="cuda") * 0.2
    b = torch.randn(Fout, device="cuda") * 0.1
    h = torch.relu(x @ w.t() + b)
    g = torch.randn(P, Fout, device="cuda")
    dx, dw, db = _C.feature_relu_backward(g, h, x, w)
    rd = (g * (h > 0)).double()
    assert dx.shape == x.shape and dw.shape == w.shape and db.shape == (Fout,)
    if P:
        ref_dx, scale = rd @ w.double(), rd.abs() @ w.double().abs()
        assert float(((dx.double() - ref_dx).abs() - 1e-5 * scale).max().clamp_min(0)) == 0.0
    rw, rb = rd.t() @ x.double(), rd.sum(0)
    sw = (rd.abs().t() @ x.double().abs()).max().clamp_min(1e-30) if P else torch.tensor(1.0)
    sb = rd.abs().sum(0).max().clamp_min(1e-30) if P else torch.tensor(1.0)
    assert float((dw.double() - rw).abs().max() / sw) <= 1e-5
    assert float((db.double() - rb).abs().max() / sb) <= 1e-5
    # the forward kernel: h to 1e-5 of its |terms| sum (exact zeros where the ReLU clips)
    hf = _C.feature_relu_forward(x, w, b)[0]
    hf2, hbf = _C.feature_relu_forward(x, w, b, with_hb=True)  # + the bf16 copy the bf16 heads block reads
    assert torch.equal(hf2, hf) and hbf.dtype == torch.bfloat16 and torch.equal(hbf, hf.to(torch.bfloat16))
    if P:
        ref_h = (x.double() @ w.double().t() + b.double())
        hscale = x.double().abs() @ w.double().abs().t() + b.double().abs()
        assert float(((hf.double() - ref_h.clamp_min(0)).abs() - 1e-5 * hscale).max().clamp_min(0)) == 0.0
    # the autograd Function end to end
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    ha = _FeatureReLU.apply(xa, wa, ba)
    torch.testing.assert_close(ha, hf, rtol=0, atol=0)
    ha.backward(g)
    ex, ew, eb = _C.feature_relu_backward(g, ha.detach(), x, w)  # same mask as the Function's (its own h)
    torch.testing.assert_close(xa.grad, ex, rtol=0, atol=0)    # deterministic: bitwise
    torch.testing.assert_close(wa.grad, ew, rtol=0, atol=0)
    torch.testing.assert_close(ba.grad, eb, rtol=0, atol=0)


@pytest.mark.parametrize("P,W,H", [(20000, 320, 240),
                                   (25000, 800, 800)])   # BASELINE C3 shape: D-NeRF standup, ~25k points
def test_train_step_fused_matches_torch_tail(P, W, H):
    """One fine-stage step through deformation + rasterizer + loss + densification statistics, fused
    (HexPlane kernel, L1 kernel, stats kernel) vs the reference's torch formulation.  The optimizer is
    held back (iteration >= opt.iterations) so the parameter gradients themselves are compared; the
    optimizer has its own test above.  Tolerance: 1e-3 of each gradient tensor's max (1e-4 at the 99.9th
    percentile)."""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    hyper, opt = config.dynerf()
    opt.iterations = 0
    pts, cols = make_point_cloud(P, seed=5)
    views = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")
    runs = []
    for fused in (False, True):
        torch.manual_seed(7)
        g = GaussianModel(3, hyper, fused=fused)
        g.create_from_pcd(pts, cols, 1.0)
        g._deformation.deformation_net.grid.fused = fused
        g._deformation.deformation_net.fused_heads = fused
        g.training_setup(opt)
        g.active_sh_degree = 3
        loss = float(train_step(g, views, opt, hyper, 3001, bg))
        grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            grads[name] = getattr(g, name).grad.detach().clone()
        runs.append((g, loss, grads))
    (ga, la, gra), (gb, lb, grb) = runs
    assert abs(lb - la) <= 1e-5 * abs(la)
    assert gra.keys() == grb.keys()
    for k in gra:
        a, b = gra[k], grb[k]
        scale = max(a.abs().max().item(), 1e-30)
        d = (a - b).abs().flatten() / scale
        # fp32 summation order differs (MFMA heads / feature layer vs hipBLASLt, fused field vs
        # grid_sample); the step amplifies ~1e-7 output differences through the L1 sign and the blend
        # thresholds into isolated gradient elements (measured <= 1.3e-4: tools/probes/heads_fwd_delta.py),
        # so the bar is the north star's 1e-3 on the max and 1e-4 on the 99.9th percentile (a defect --
        # a wrong head, a lost bias or mask -- moves most elements by O(1))
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k
    # the statistic sums |d loss / d mean2D| per point: the same bar as the gradients above (at C3's
    # 25k points / 800x800 two isolated points move by ~2e-4 of the max: a blend-threshold flip)
    acc_scale = max(ga.xyz_gradient_accum.abs().max().item(), 1e-30)
    d = (gb.xyz_gradient_accum - ga.xyz_gradient_accum).abs().flatten() / acc_scale
    assert d.max().item() < 1e-3, d.max().item()
    assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4
    torch.testing.assert_close(gb.denom, ga.denom, rtol=0, atol=0)
    torch.testing.assert_close(gb.max_radii2D, ga.max_radii2D, rtol=0, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", ["all", "some", "none"])
def test_deform_tail_matches_torch(heads):
    """kernels.deform_tail (residual adds + cat(f_dc, f_rest) + exp / normalize / sigmoid in one HIP pass
    each way) against the reference's torch graph (scene/deformation.py:140-146, gaussian_model.py:116-118,
    gaussian_renderer/__init__.py:97-99): outputs to 1e-6 relative, every gradient to 1e-5 of its max."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from gs4d_train.kernels import deform_tail
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    P = 5003
    mk = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_(True)
    base = [mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 1), mk(P, 1, 3), mk(P, 15, 3)]
    deltas = [mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 1), mk(P, 48)]
    if heads == "some":
        deltas[1] = deltas[3] = None
    elif heads == "none":
        deltas = [None] * 5
    ups = [torch.randn(P, 3, generator=g).to(dev), torch.randn(P, 3, generator=g).to(dev),
           torch.randn(P, 4, generator=g).to(dev), torch.randn(P, 1, generator=g).to(dev),
           torch.randn(P, 16, 3, generator=g).to(dev)]
    leaves = base + [d for d in deltas if d is not None]
    out = deform_tail(*base, *deltas)
    ga = torch.autograd.grad(sum((o * u).sum() for o, u in zip(out, ups)), leaves)
    xyz, s, r, o, fdc, frest = base
    add = lambda a, b: a if b is None else a + b
    sh = torch.cat((fdc, frest), dim=1)
    ref = (add(xyz, deltas[0]), torch.exp(add(s, deltas[1])), torch.nn.functional.normalize(add(r, deltas[2])),
           torch.sigmoid(add(o, deltas[3])), sh if deltas[4] is None else sh + deltas[4].reshape(P, 16, 3))
    gb = torch.autograd.grad(sum((x * u).sum() for x, u in zip(ref, ups)), leaves)
    for a, b in zip(out, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    for a, b in zip(ga, gb):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-20)


def test_train_step_bf16_mlp_tracks_fp32():
    """The opt-in bf16 deformation MLP (hyper.mlp_dtype = "bf16", BASELINE C3's "bf16/fp32"): one fused
    fine-stage step at C3's shape against the fp32 step from the same state.  bf16 operands carry 8
    mantissa bits, so the bar is statistical: loss within 1 %, every parameter-gradient tensor within 5 %
    of its norm (relative L2; measured <= 2.4 %, the means' gradient, which also flows through the
    deformation)."""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    pts, cols = make_point_cloud(25000, seed=5)
    views = make_training_views(2, 800, 800, seed=6)
    bg = torch.ones(3, device="cuda")
    runs = []
    for dtype in ("fp32", "bf16"):
        hyper, opt = config.dynerf()
        hyper.mlp_dtype = dtype
        opt.iterations = 0
        torch.manual_seed(7)
        g = GaussianModel(3, hyper, fused=True)
        g.create_from_pcd(pts, cols, 1.0)
        g._deformation.deformation_net.grid.fused = True
        g._deformation.deformation_net.fused_heads = True
        g.training_setup(opt)
        g.active_sh_degree = 3
        loss = float(train_step(g, views, opt, hyper, 3001, bg))
        grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            grads[name] = getattr(g, name).grad.detach().clone()
        runs.append((loss, grads))
    (la, ga), (lb, gb) = runs
    assert abs(lb - la) <= 1e-2 * abs(la), (la, lb)
    assert ga.keys() == gb.keys()
    for k in ga:
        assert gb[k].dtype == torch.float32, k
        rel = float((gb[k] - ga[k]).norm() / ga[k].norm().clamp_min(1e-30))
        assert rel <= 5e-2, (k, rel)


def test_heads_block_forward_lds_fallback(monkeypatch):
    """A device that cannot give the heads block forward its LDS (status 4, GS4D_TRAIN_ERR_LDS) makes the
    wrapper warn once and use the GEMM formulation on that device from then on: same outputs and gradients
    as the block pass to fp32 rounding (simulated: the binding raises as it would)."""
    from gs4d_train import _C, deformation as D
    torch.manual_seed(5)
    P, W, ns = 3000, 128, [3, 3, 4, 1, 48]
    k = len(ns)
    h = torch.relu(torch.randn(P, W, device="cuda"))
    w1 = (torch.randn(k * W, W, device="cuda") / W ** 0.5).requires_grad_(True)
    b1 = (torch.randn(k * W, device="cuda") * 0.1).requires_grad_(True)
    second = []
    for n in ns:
        second += [(torch.randn(n, W, device="cuda") / W ** 0.5).requires_grad_(True),
                   torch.randn(n, device="cuda").requires_grad_(True)]
    gs = [torch.randn(P, n, device="cuda") for n in ns]

    def run():
        outs = D._DeformHeads.apply(True, h, w1, b1, *second)
        torch.autograd.backward(outs, gs)
        grads = [t.grad.clone() for t in [w1, b1] + second]
        for t in [w1, b1] + second:
            t.grad = None
        return [o.detach() for o in outs], grads

    ref_out, ref_grad = run()
    real = _C.heads_block_forward

    def refuse(*args):
        raise RuntimeError("heads_block_forward failed (status 4)")
    monkeypatch.setattr(_C, "heads_block_forward", refuse)
    try:
        with pytest.warns(UserWarning, match="heads block forward unavailable"):
            out, grad = run()
        assert h.device.index in D._NO_BLOCK_FORWARD
        out2, _ = run()  # no second attempt, no second warning
    finally:
        D._NO_BLOCK_FORWARD.discard(h.device.index)
        monkeypatch.setattr(_C, "heads_block_forward", real)
    for a, b in zip(out + out2, ref_out + ref_out):
        assert float((a - b).abs().max()) <= 1e-4 * max(float(b.abs().max()), 1.0)
    for a, b in zip(grad, ref_grad):
        assert float((a - b).abs().max()) <= 1e-4 * max(float(b.abs().max()), 1e-20)


def test_zero_points_sink_is_a_fresh_leaf():
    """render()'s means2D gradient sink (gaussian_renderer/__init__.py:24-29): one kept zero buffer, but every
    call a new leaf with its own .grad, so one step's viewspace gradient never leaks into another's."""
    from gs4d_train.render import _zero_points
    xyz = torch.rand(10, 3, device="cuda")
    a, b = _zero_points(xyz), _zero_points(xyz)
    assert a is not b and a.is_leaf and b.is_leaf and a.requires_grad and b.requires_grad
    assert not bool(torch.any(a)) and a.shape == xyz.shape and a.dtype == xyz.dtype
    (a * 2.0).sum().backward()
    assert b.grad is None and torch.equal(a.grad, torch.full_like(a, 2.0))
    (b * 3.0).sum().backward()
    assert torch.equal(a.grad, torch.full_like(a, 2.0)) and torch.equal(b.grad, torch.full_like(b, 3.0))
    assert not bool(torch.any(_zero_points(xyz)))


def test_hexplane_points_alias_sums_xyz_gradient_bitwise():
    """kernels.hexplane_points with alias: xyz's other use (the deformation tail's xyz + dx) reads the pass-through
    view, and the points' backward sums that use's gradient into its own pass -- bitwise the gradient autograd
    forms with its separate add.  A use of the view alone (no field gradient) still gets its gradient."""
    from gs4d_train.kernels import hexplane_points
    torch.manual_seed(11)
    P = 5003
    x0 = torch.randn(P, 3, device="cuda")
    t = torch.full((1, 1), 0.3, device="cuda").expand(P, 1)
    aabb = torch.tensor([[1.5, 1.2, 1.3], [-1.4, -1.1, -1.6]], device="cuda")
    w, u = torch.randn(P, 4, device="cuda"), torch.randn(P, 3, device="cuda")
    xa = x0.clone().requires_grad_(True)
    ((hexplane_points(xa, t, aabb) * w).sum() + (xa * u).sum()).backward()
    xb = x0.clone().requires_grad_(True)
    alias = []
    pts = hexplane_points(xb, t, aabb, alias)
    assert len(alias) == 1 and alias[0].data_ptr() == xb.data_ptr()
    ((pts * w).sum() + (alias[0] * u).sum()).backward()
    assert torch.equal(xa.grad, xb.grad)
    xc = x0.clone().requires_grad_(True)
    alias = []
    hexplane_points(xc, t, aabb, alias)
    (alias[0] * u).sum().backward()
    assert torch.equal(xc.grad, u)
