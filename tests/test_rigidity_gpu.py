"""The exact K-NN graph (simple_knn._C.knn_graph), the fused local-isometry term (gs4d_train.rigidity) and the layers
that use them (render(return_means=True), Rigidity.graph_for, train_step(rigidity=...)) on the GPU.

Graph: torch.equal against the numpy brute force of tests/rigidity_refs.py (indices, distance bits, transpose).
Loss: per tensor T in (value, dL/dxa, dL/dxb), e = max |T - T64| / max |T64| against the fp64 torch graph; the fused
e_f must not exceed max(4 e_u, 1e-6), e_u being the unfused fp32 torch formulation's error measured in the same test
on the same GPU (the deformation-route tests' bar).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import rigidity_refs as RR
import stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def knn_graph(x, K):
    from simple_knn._C import knn_graph as f
    t = x if torch.is_tensor(x) else torch.from_numpy(np.array(x))
    return f(t.to(DEV), K)


def dist_cuda2(x):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.from_numpy(np.array(x)).to(DEV))


def assert_graph(got, want, tag):
    for name, g, w in zip(("idx", "dist2", "in_start", "in_edge"), got, want):
        w = torch.from_numpy(np.array(w))
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape)
        if name == "dist2":
            g, w = g.view(torch.int32), w.view(torch.int32)
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(-1))
            k = int(bad[0])
            raise AssertionError(f"{tag}: {name} differs in {len(bad)} places, first at {k}: "
                                 f"{g.reshape(-1)[k].item()} against {w.reshape(-1)[k].item()}")


# ---- the graph ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8, 16])
@pytest.mark.parametrize("name", RR.CLOUDS)
def test_graph_is_exact(name, K):
    assert_graph(knn_graph(RR.cloud(name), K), RR.knn_of(name, K), f"{name} K={K}")


@pytest.mark.parametrize("K", [8, 16])
def test_graph_edge_sizes(K):
    rng = np.random.default_rng(11)
    for P in (1, 2, 3, 4, 9, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097):
        x = rng.normal(size=(P, 3)).astype(np.float32)
        idx, dist = RR.knn_rows(x, K, np.arange(P))
        assert_graph(knn_graph(x, K), (idx, dist, *RR.transpose(idx)), f"P={P} K={K}")
        if P - 1 < K:
            assert (idx[:, P - 1:] == -1).all() and (dist[:, P - 1:] == RR.FLT_MAX).all()
    idx, dist, in_start, in_edge = knn_graph(np.zeros((0, 3), np.float32), K)
    assert idx.shape == (0, K) and dist.shape == (0, K) and in_edge.shape == (0,)
    assert in_start.cpu().tolist() == [0]


def _mean3(dist):
    d = dist.cpu()
    return (d[:, 0] + d[:, 1] + d[:, 2]) / 3.0


@pytest.mark.parametrize("name", RR.CLOUDS)
def test_graph_agrees_with_distCUDA2(name):
    x = RR.cloud(name)
    got = _mean3(knn_graph(x, 3)[1])
    assert torch.equal(got.view(torch.int32), dist_cuda2(x).cpu().view(torch.int32))


def test_graph_large_clustered_cloud():
    x = RR.large_clustered()
    P = x.shape[0]
    idx, dist, in_start, in_edge = knn_graph(x, 8)
    d3 = knn_graph(x, 3)[1]
    assert torch.equal(_mean3(d3).view(torch.int32), dist_cuda2(x).cpu().view(torch.int32))
    assert torch.equal(d3.cpu(), dist[:, :3].cpu())
    rows = np.random.default_rng(1).choice(P, 256, replace=False)
    ridx, rdist = RR.knn_rows(x, 8, rows)
    assert np.array_equal(idx.cpu().numpy()[rows], ridx)
    assert np.array_equal(dist.cpu().numpy()[rows].view(np.int32), rdist.view(np.int32))
    # every row: ascending by (distance, index), free of self and of repeats
    i64, d = idx.long(), dist
    assert bool((i64 >= 0).all() and (i64 < P).all())
    assert bool((i64 != torch.arange(P, device=DEV)[:, None]).all())
    up = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i64[:, 1:] > i64[:, :-1]))
    assert bool(up.all())  # strictly ascending pairs: no repeats either
    # the transpose lists every edge once, under its target, in ascending edge id
    e = in_edge.long()
    assert int(in_start[0]) == 0 and int(in_start[-1]) == 8 * P
    assert torch.equal(torch.sort(e).values, torch.arange(8 * P, device=DEV))
    tgt = i64.reshape(-1)[e]
    assert bool((tgt[1:] >= tgt[:-1]).all()) and bool(((tgt[1:] > tgt[:-1]) | (e[1:] > e[:-1])).all())
    assert torch.equal(torch.bincount(tgt, minlength=P), (in_start[1:] - in_start[:-1]).long())


def _graph_case_inputs(seed):
    """4097 normal points with 200 duplicated rows (ties decided by the index), another draw per seed"""
    x = np.random.default_rng(seed + 21).normal(size=(4097, 3)).astype(np.float32)
    x[-200:] = x[:200]
    return SC._od(x=torch.tensor(x))


GRAPH_CASE = SC.Case("knn_graph", ("knn_graph",), _graph_case_inputs,
                     lambda t: list(knn_graph(t["x"], 8)) + list(knn_graph(t["x"], 16)))


@pytest.fixture(scope="module")
def side_streams():
    cal = SC.calibration("cuda:0")
    first = cal.fresh_stream()
    return first, cal.fresh_stream(apart_from=(first,))


def test_graph_two_calls_and_side_stream(side_streams):
    x = RR.cloud("hub")
    a, b = knn_graph(x, 8), knn_graph(x, 8)
    assert SC.first_difference(list(a), list(b)) is None
    SC.run_case(GRAPH_CASE, side_streams[0], probe_stream=side_streams[1])


def test_graph_refuses_bad_input():
    from simple_knn._C import knn_graph as f
    for bad in (lambda: f(torch.zeros(4, 2, device=DEV), 8), lambda: f(torch.zeros(4, 3), 8),
                lambda: f(torch.zeros(4, 3, device=DEV), 0), lambda: f(torch.zeros(4, 3, device=DEV), 17)):
        with pytest.raises(RuntimeError):
            bad()


# ---- the loss -------------------------------------------------------------------------------------------------------
def _graph_of(name, K, weights):
    from gs4d_train.rigidity import KnnGraph
    idx, dist, in_start, in_edge = (torch.from_numpy(np.array(a)).to(DEV) for a in RR.knn_of(name, K))
    w = None
    if weights:
        w = torch.where(idx >= 0, torch.exp(-2.0 * dist), torch.zeros_like(dist))
    return KnnGraph(idx, dist, in_start, in_edge, w)


LOSS_CASES = [("gauss", 8), ("lattice", 8), ("hub", 8), ("gauss", 1), ("gauss", 16)]


@pytest.mark.parametrize("weights", [False, True], ids=["ones", "exp"])
@pytest.mark.parametrize("name,K", LOSS_CASES)
def test_loss_matches_fp64_within_the_unfused_bar(name, K, weights):
    """measured on an MI355X (e_f / e_u per tensor) in DESIGN 10.15"""
    from gs4d_train.rigidity import isometry_loss_and_grad
    g = _graph_of(name, K, weights)
    xa, xb = (t.to(DEV) for t in RR.loss_inputs(name))
    fused = isometry_loss_and_grad(xa, xb, g, 1.0)
    r64 = RR.isometry_value_and_grads(xa, xb, g.idx, g.weights, torch.float64)
    r32 = RR.isometry_value_and_grads(xa, xb, g.idx, g.weights, torch.float32)
    figures = []
    for tensor, f, u, r in zip(("value", "dxa", "dxb"), fused, r32, r64):
        figures.append((tensor, RR.rel_err(f, r), RR.rel_err(u, r)))
    print(f"[rigidity] {name} K={K} weights={'exp' if weights else 'ones'}: " +
          ", ".join(f"{t} e_f {ef:.2e} e_u {eu:.2e}" for t, ef, eu in figures), flush=True)
    for t, ef, eu in figures:
        assert ef <= max(4 * eu, 1e-6), (t, ef, eu)


def test_loss_identities():
    from gs4d_train import _C
    from gs4d_train.rigidity import KnnGraph, isometry_loss_and_grad
    g = _graph_of("hub", 8, True)
    xa, xb = (t.to(DEV) for t in RR.loss_inputs("hub"))
    # xb == xa: value 0 and zero gradients exactly
    v, ga, gb = isometry_loss_and_grad(xa, xa.clone(), g, 1.0)
    assert float(v) == 0.0 and not ga.any() and not gb.any()
    # two calls: the same bits
    full = isometry_loss_and_grad(xa, xb, g, 0.37)
    assert SC.first_difference(list(isometry_loss_and_grad(xa, xb, g, 0.37)), list(full)) is None
    # a NULL side gives the other side the full call's bits
    call = lambda a, b: _C.isometry_loss_grad(g.idx, g.in_start, g.in_edge, g.weights, xa, xb, 0.37, a, b)
    va, only_a, none_b = call(True, False)
    vb, none_a, only_b = call(False, True)
    vn, na, nb = call(False, False)
    assert none_b is None and none_a is None and na is None and nb is None
    assert SC.first_difference([va, only_a, vb, only_b, vn], [full[0], full[1], full[0], full[2], full[0]]) is None
    # weights = None equals a tensor of ones, bitwise (ones also in the empty slots: they are skipped by the index)
    g1 = _graph_of("hub", 8, False)
    ones = isometry_loss_and_grad(xa, xb, KnnGraph(g1.idx, g1.dist2, g1.in_start, g1.in_edge, torch.ones_like(g1.dist2)), 1.0)
    assert SC.first_difference(list(ones), list(isometry_loss_and_grad(xa, xb, g1, 1.0))) is None


def _loss_case_inputs(seed):
    """4097 points, K = 8, with 200 duplicated rows (zero distances) and weights"""
    x = np.random.default_rng(seed + 31).normal(size=(4097, 3)).astype(np.float32)
    x[-200:] = x[:200]
    idx = RR.knn_rows(x, 8, np.arange(4097))[0]
    in_start, in_edge = RR.transpose(idx)
    g = SC._g(seed)
    xa = torch.tensor(x)
    return SC._od(xa=xa, xb=xa + 0.05 * torch.randn(4097, 3, generator=g), w=torch.rand(4097, 8, generator=g),
                  idx=torch.tensor(idx), in_start=torch.tensor(in_start), in_edge=torch.tensor(in_edge))


def _loss_case_call(t):
    from gs4d_train import _C
    out = list(_C.isometry_loss_grad(t["idx"], t["in_start"], t["in_edge"], t["w"], t["xa"], t["xb"], 0.5, True, True))
    return out + [_C.isometry_loss_grad(t["idx"], t["in_start"], t["in_edge"], None, t["xa"], t["xb"], 1.0, False, False)[0]]


LOSS_CASE = SC.Case("isometry_loss_grad", ("isometry_loss_grad",), _loss_case_inputs, _loss_case_call)


def test_loss_on_a_side_stream(side_streams):
    SC.run_case(LOSS_CASE, side_streams[0], probe_stream=side_streams[1])


def test_autograd_function_matches_the_fp64_graph():
    from gs4d_train.rigidity import build_graph, isometry_loss
    P, K = 65, 8
    x = torch.from_numpy(np.random.default_rng(2).normal(size=(P, 3)).astype(np.float32)).to(DEV)
    g = build_graph(x, K, weight_lambda=2.0)
    ridx = RR.knn_rows(x.cpu().numpy(), K, np.arange(P))[0]
    assert np.array_equal(g.idx.cpu().numpy(), ridx)
    assert torch.equal(g.weights, torch.exp(-2.0 * g.dist2))
    assert build_graph(x, K).weights is None
    xb = x + 0.05 * torch.randn(P, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    up = 1.7
    r64 = RR.isometry_value_and_grads(x, xb, g.idx, g.weights, torch.float64)
    r32 = RR.isometry_value_and_grads(x, xb, g.idx, g.weights, torch.float32)
    a, b = x.clone().requires_grad_(True), xb.clone().requires_grad_(True)
    v = isometry_loss(a, b, g)
    (v * up).backward()
    for name, f, u, r in (("value", v, r32[0], r64[0]), ("dxa", a.grad, r32[1] * up, r64[1] * up),
                          ("dxb", b.grad, r32[2] * up, r64[2] * up)):
        ef, eu = RR.rel_err(f, r), RR.rel_err(u, r)
        print(f"[rigidity] autograd P=65 {name}: e_f {ef:.2e} e_u {eu:.2e}", flush=True)
        assert ef <= max(4 * eu, 1e-6), (name, ef, eu)
    # only the side that requires grad is asked for and receives one
    a2, b2 = x.clone(), xb.clone().requires_grad_(True)
    isometry_loss(a2, b2, g).backward()
    assert a2.grad is None and RR.rel_err(b2.grad * up, b.grad) <= 1e-6


def test_value_errors():
    from gs4d_train.rigidity import build_graph, isometry_loss, isometry_loss_and_grad
    x = torch.randn(65, 3, device=DEV)
    g = build_graph(x, 4)
    for bad in (lambda: isometry_loss(x, x[:64], g), lambda: isometry_loss(x[:, :2], x[:, :2], g),
                lambda: isometry_loss(x.double(), x.double(), g), lambda: isometry_loss(x, x.cpu(), g),
                lambda: isometry_loss(x.cpu(), x.cpu(), g), lambda: isometry_loss(x[:64], x[:64], g),
                lambda: isometry_loss_and_grad(x[:64], x[:64], g, 1.0)):
        with pytest.raises(ValueError):
            bad()


# ---- the layers -----------------------------------------------------------------------------------------------------
def _model(fused, P=3000, seed=7, iterations=0, moving=False):
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud
    hyper, opt = config.dynerf()
    opt.iterations = iterations
    pts, cols = make_point_cloud(P, seed=5)
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=fused)
    if moving:
        # a fresh position head moves nothing (its last layer starts near zero) and the term would vanish with its
        # gradient: give the head an output of the order of the neighbour distances
        last = g._deformation.deformation_net.pos_deform[-1]
        with torch.no_grad():
            last.weight.add_(1.0 * torch.randn(last.weight.shape, generator=torch.Generator().manual_seed(9)))
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = fused
    g._deformation.deformation_net.fused_heads = fused
    g.training_setup(opt)
    g.active_sh_degree = 3
    return g, hyper, opt


def _views(n=2):
    from gs4d_train.synthetic import make_training_views
    return make_training_views(n, 96, 64, seed=6)


def _grads(g):
    out = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        out[name] = getattr(g, name).grad.detach().clone()
    return out


def test_render_returns_the_rasterizers_means(monkeypatch):
    import diff_gaussian_rasterization as dgr
    from gs4d_train.render import render
    g, hyper, opt = _model(True)
    cam = _views(1)[0][0]
    bg = torch.ones(3, device=DEV)
    seen = []
    forward = dgr.GaussianRasterizer.forward

    def spy(self, *args, **kw):
        seen.append(kw["means3D"])
        return forward(self, *args, **kw)

    monkeypatch.setattr(dgr.GaussianRasterizer, "forward", spy)
    plain = render(cam, g, False, bg, stage="fine")
    assert set(plain.keys()) == {"render", "viewspace_points", "radii", "depth", "visibility_filter"}
    pkg = render(cam, g, False, bg, stage="fine", return_means=True)
    assert set(pkg.keys()) == set(plain.keys()) | {"means3D"}
    assert pkg["means3D"] is seen[-1] and pkg["means3D"].requires_grad and pkg["means3D"].shape == g.get_xyz.shape
    assert torch.equal(pkg["render"], plain["render"])
    coarse = render(cam, g, False, bg, stage="coarse", return_means=True)
    assert torch.equal(coarse["means3D"], g.get_xyz)


def test_graph_for_rebuilds_when_the_rows_change_or_the_interval_passes():
    from gs4d_train.rigidity import Rigidity
    g, hyper, opt = _model(True, P=500)
    r = Rigidity(K=4, weight_lambda=2.0, refresh_interval=100)
    g0 = r.graph_for(g, 3000)
    assert r.builds == 1 and g0.P == 500 and g0.K == 4 and g0.weights is not None
    assert r.graph_for(g, 3001) is g0 and r.graph_for(g, 3099) is g0 and r.builds == 1
    g1 = r.graph_for(g, 3100)  # the interval has passed
    assert r.builds == 2 and g1 is not g0
    mask = torch.zeros(500, dtype=torch.bool, device=DEV)
    mask[::5] = True
    g.prune_points(mask)
    g2 = r.graph_for(g, 3101)
    assert r.builds == 3 and g2.P == 400
    # the same row count with other rows (a prune and a clone would do this): the generation counter sees it
    gen = g.row_generation
    from gs4d_train import surgery
    surgery.apply(g, surgery.RowPlan(keep=torch.arange(400, device=DEV).flip(0)))
    assert g.row_generation == gen + 1 and g.get_xyz.shape[0] == 400
    assert r.graph_for(g, 3102) is not g2 and r.builds == 4
    assert r.graph_for(g, 3103) is r.graph and r.builds == 4


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_train_step_adds_the_term(fused):
    """the step with lambda_rigid against the step without it plus the term by hand (the fp32 torch formulation on the
    render's own means3D): the loss, and every parameter gradient within the train-step tests' fused-against-unfused
    bar (1e-3 of the tensor's max, 1e-4 at the 99.9th percentile)"""
    from gs4d_train.render import render
    from gs4d_train.rigidity import Rigidity
    from gs4d_train.train import train_step
    views = _views(2)
    bg = torch.ones(3, device=DEV)
    lam = 0.1
    ga, hyper, opt = _model(fused, moving=True)
    opt.lambda_rigid = lam
    rig = Rigidity(K=8, weight_lambda=2.0)
    loss_a = float(train_step(ga, views, opt, hyper, 3001, bg, rigidity=rig))
    assert rig.builds == 1
    grads_a = _grads(ga)
    gb, hyper, opt_b = _model(fused, moving=True)
    loss_b = float(train_step(gb, views, opt_b, hyper, 3001, bg))
    grads_b = _grads(gb)
    gb.optimizer.zero_grad(set_to_none=True)
    term = 0.0
    for view in views:
        m = render(view[0], gb, False, bg, stage="fine", return_means=True)["means3D"]
        t = RR.isometry_torch(gb.get_xyz, m, rig.graph.idx, rig.graph.weights) * (lam / len(views))
        t.backward()
        term += float(t.detach())
    hand = {n: p.grad for n, p in gb._deformation.named_parameters() if p.grad is not None}
    hand["_xyz"] = gb._xyz.grad
    print(f"[rigidity] train_step fused={fused}: loss {loss_a:.6f} = {loss_b:.6f} + {term:.6f}", flush=True)
    assert term > 0 and abs(loss_a - (loss_b + term)) <= 1e-5 * abs(loss_b + term)
    assert grads_a.keys() == grads_b.keys()
    moved = 0
    for k in grads_a:
        want = grads_b[k] + hand[k] if hand.get(k) is not None else grads_b[k]
        moved += int(hand.get(k) is not None and bool(hand[k].any()))
        scale = max(want.abs().max().item(), 1e-30)
        d = (grads_a[k] - want).abs().flatten() / scale
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert d.kthvalue(max(1, int(0.999 * d.numel()))).values.item() < 1e-4, k
    assert moved >= 3  # the term reaches the canonical means, the field and the position head
    # the term's share of the canonical means' gradient stands five times above the 1e-3 bar: the check above would
    # miss a lost term only if the share were below that bar
    share = hand["_xyz"].abs().max().item() / max((grads_b["_xyz"] + hand["_xyz"]).abs().max().item(), 1e-30)
    print(f"[rigidity] train_step fused={fused}: the term's share of max |dL/dxyz| {share:.2e}", flush=True)
    assert share > 5e-3


def test_train_step_without_rigidity_is_unchanged():
    from gs4d_train.rigidity import Rigidity
    from gs4d_train.train import train_step
    views = _views(2)
    bg = torch.ones(3, device=DEV)
    params = []
    rig = Rigidity(K=8)
    for kw, lam in (({}, 0.0), ({"rigidity": None}, 0.1), ({"rigidity": rig}, 0.0)):
        g, hyper, opt = _model(True, iterations=30_000)
        opt.lambda_rigid = lam
        loss = train_step(g, views, opt, hyper, 3001, bg, **kw)
        params.append([loss] + [p.detach().clone() for grp in g.optimizer.param_groups for p in grp["params"]])
    assert rig.builds == 0
    for other in params[1:]:
        assert SC.first_difference(other, params[0]) is None
    # the coarse stage never adds the term
    g, hyper, opt = _model(True, iterations=30_000)
    opt.lambda_rigid = 0.1
    train_step(g, views, opt, hyper, 100, bg, stage="coarse", rigidity=rig)
    assert rig.builds == 0


def test_train_step_needs_means3D_from_render_fn():
    from gs4d_train.render import render
    from gs4d_train.rigidity import Rigidity
    from gs4d_train.train import train_step
    g, hyper, opt = _model(True)
    opt.lambda_rigid = 0.1

    def render_fn(cam, pc, debug, bg, stage="fine", return_means=False, **kw):
        return render(cam, pc, debug, bg, stage=stage, **kw)

    with pytest.raises(RuntimeError, match="return_means"):
        train_step(g, _views(1), opt, hyper, 3001, torch.ones(3, device=DEV), render_fn=render_fn, rigidity=Rigidity())
