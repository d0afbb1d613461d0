"""GPU tests of the per-Gaussian blend-weight importance (gs4d_importance and everything above it).

Two references (tests/importance_refs.py).  The forward itself, through one-hot colours: channel c of the image is
w_ip = alpha_ip T_ip of the chosen Gaussian, bit for bit, so weight_max and pixel_count are compared exactly on every
scene, termination, the cap and the 1/255 rule included.  And the fp64 restatement, on the scenes where no rule is
near its threshold (tests/test_depth_grad_boundary.py asserts that).

The bound on weight_sum against the one-hot image (test 1).  Let a Gaussian blend into n = pixel_count pixels with
weights w_1 .. w_n >= 0 (floats) and S = sum w (exact; the test forms it in fp64 from the image, where n <= 2^16 terms
of 24 bits each add exactly).  Any summation order is a binary tree of additions; an addition with a zero operand is
exact, and each rounding addition fl(a + b) = (a + b)(1 + d), |d| <= u = 2^-24, merges two non-empty sets of terms,
so a term passes through at most min(h, n - 1) rounding additions, h the tree's depth.  The computed sum is therefore
sum w_k (1 + e_k) with |e_k| <= (1 + u)^min(h, n - 1) - 1, and since every w_k >= 0 the error is at most
((1 + u)^k - 1) S with k = min(h, n - 1).  The kernel's tree has h = 2 (a lane's four pixels) + 6 (the wave) + 6 (the
segmented scan) + the waves a Gaussian's slots span (5 at most here).  Since (1 + u)^k - 1 <= k u (1 + k u) for k u < 1
and k + 1 <= n, the error is within n u S whenever k^2 u <= 1, that is k <= 4096: every h here and in any image of
fewer than a quarter of a million tiles.  The bar n u S uses nothing of the order beyond that: it is no measured
tolerance.

The identity with the alpha image (test 3).  Per pixel the forward computes w_k = fl(a_k T_k) and T_{k+1} =
fl(T_k fl(1 - a_k)), and exactly a_k T_k + T_k (1 - a_k) = T_k, so w_k + T_{k+1} = T_k + e_k with |e_k| <= u (w_k +
2 T_{k+1}): over the K contributors sum_k w_k = 1 - T_K + sum e_k, |sum e_k| <= u (A + 2 K) with A the pixel's alpha,
and the alpha image adds u A for its own subtraction.  Over the image: |sum_p sum_k w - sum_p alpha_p| <=
u (2 total + 2 C), C = sum_p K_p = sum_i pixel_count_i the number of blended pairs and total = sum_p alpha_p.  The
fp32 per-Gaussian sums add at most Nmax u total by the bound above (Nmax the largest pixel_count).  On scenes whose
pairs-per-unit-alpha C / total does not exceed (3 Kmax - 2) / 2 -- asserted, from the GPU's own counts, before the
identity is -- this is within (3 Kmax + Nmax) u total, Kmax the largest n_contrib, the bar of the test.
"""
import math

import numpy as np
import pytest
import torch

import alpha_scenes as AS
import depth_scenes as DS
import importance_refs as IR
from gpu_helpers import to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _scene(name):
    if name == "stack":
        return dict(s=IR.stack_scene(), colors=None, cov3D=None, use_sh=True)
    if name == "wide":
        return dict(s=IR.wide_scene(), colors=None, cov3D=None, use_sh=True)
    if name == "sparse_culled":
        return dict(s=IR.sparse_culled_scene(), colors=None, cov3D=None, use_sh=True)
    return AS.scene(name) if name in AS.NAMES else DS.scene(name)


def _forward(sc, d, colors, cov3D, aa=False):
    s = sc["s"]
    e = torch.empty(0, device=d["means3D"].device)
    args = (d["bg"], d["means3D"], e if colors is None else colors, d["opacities"],
            e if cov3D is not None else d["scales"], e if cov3D is not None else d["rotations"],
            float(s["scale_modifier"]), e if cov3D is None else cov3D, d["viewmatrix"], d["projmatrix"],
            float(s["tanfovx"]), float(s["tanfovy"]), int(s["H"]), int(s["W"]), d["shs"] if sc["use_sh"] else e,
            int(s["sh_degree"]), d["campos"], False, False)
    return _C().rasterize_gaussians_aa(*args, True) if aa else _C().rasterize_gaussians(*args)


def _importance(sc, fwd):
    s = sc["s"]
    return _C().gaussian_importance(fwd[4], fwd[5], fwd[6], fwd[0], len(s["means3D"]), int(s["H"]), int(s["W"]))


def gpu(name, aa=False):
    """device tensors, the HIP forward of a scene and the scores of that forward, made once"""
    key = (name, aa)
    if key not in _GPU:
        sc = _scene(name)
        dev = torch.device("cuda:0")
        d = to_dev(sc["s"], dev)
        colors = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
        cov3D = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
        fwd = _forward(sc, d, colors, cov3D, aa)
        _GPU[key] = dict(sc=sc, d=d, colors=colors, cov3D=cov3D, fwd=fwd, scores=_importance(sc, fwd))
    return _GPU[key]


def _check_onehot(name, ids, aa=False):
    """the scores of Gaussians `ids` against their one-hot images: max and count exact, sum within n u S"""
    g = gpu(name, aa)
    wsum, wmax, count = (t.cpu() for t in g["scores"])
    ref = IR.onehot_scores(_C(), g["sc"]["s"], g["d"], ids, cov3D=g["cov3D"], antialiasing=aa)
    idx = torch.tensor(ref["ids"], dtype=torch.long)
    assert torch.equal(wmax[idx], ref["max"]), f"{name}: weight_max differs from the forward's own weights"
    assert torch.equal(count[idx].long(), ref["count"]), f"{name}: pixel_count differs from the forward's"
    err = (wsum[idx].double() - ref["sum"]).abs()
    bar = IR.sum_bound(ref["count"], ref["sum"])
    assert bool((err <= bar).all()), f"{name}: weight_sum off by up to {float((err / bar.clamp_min(1e-300)).max()):.3f} of n u S"
    used = float((err[bar > 0] / bar[bar > 0]).max()) if bool((bar > 0).any()) else 0.0
    return ref, used


# ---- 1. exact against the forward itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small0", "hi0", "dense0", "cov3D5", "opaque", "sparse"])
def test_scores_are_the_forwards_own_weights(name):
    P = len(_scene(name)["s"]["means3D"])
    ref, used = _check_onehot(name, range(P))
    blended = int((ref["count"] > 0).sum())
    print(f"\n[importance] {name}: {blended} of {P} Gaussians blend, largest count {int(ref['count'].max())}, "
          f"largest max {float(ref['max'].max()):.4f}, sum error at most {used:.3f} of n u S")
    assert blended >= (5 if name == "sparse" else 40)


def _stack_lists():
    g = gpu("stack")
    s = g["sc"]["s"]
    out = _C().debug_tile_lists(g["fwd"][4], g["fwd"][5], g["fwd"][6], len(s["means3D"]), int(s["W"]), int(s["H"]),
                                g["fwd"][0])
    return out[0].cpu().numpy().astype(np.int64), out[3].cpu().numpy().astype(np.int64)


def test_stack_scene_first_middle_and_last_of_every_tile():
    ranges, gid = _stack_lists()
    lens = ranges[:, 1] - ranges[:, 0]
    assert lens.tolist() == IR.STACK_LENGTHS  # nothing is culled here: every sort path of the forward runs
    ids = []
    for a, b in ranges:
        if b > a:
            ids += [int(gid[a]), int(gid[(a + b - 1) // 2]), int(gid[b - 1])]
    ids = list(dict.fromkeys(ids))
    ref, used = _check_onehot("stack", ids)
    # the 513 run's centre pixel retires before the run ends (the forward's own n_contrib); the 256 run's does not
    g = gpu("stack")
    n_contrib = _n_contrib(g)[0].reshape(32, 80).cpu()
    assert 0 < int(n_contrib[24, 72]) < 513 and int(n_contrib[24, 40]) == 256
    c = dict(zip(ref["ids"], ref["count"].tolist()))
    assert c[int(gid[ranges[9, 0]])] > 0 and c[int(gid[ranges[7, 1] - 1])] > 0
    print(f"\n[importance] stack: {len(ids)} Gaussians compared, sum error at most {used:.3f} of n u S; the 513 run's "
          f"centre pixel blends {int(n_contrib[24, 72])} splats")


# ---- 2. against the fp64 restatement -------------------------------------------------------------------------------
FP64_SCENES = ["small0", "small1", "small2", "small3", "hi0", "rot0", "dense0", "dense1", "dense2", "dense3",
               "colors4", "cov3D5"]


@pytest.mark.parametrize("name", FP64_SCENES)
def test_scores_match_the_fp64_restatement(oracle, name):
    ref = DS.reference(oracle, name)
    want = IR.reference_scores(DS.scene(name)["s"], ref["export"]["point_list"], ref["export"]["ranges"])
    wsum, wmax, count = (t.cpu() for t in gpu(name)["scores"])
    assert torch.equal(count.long(), want["count"]), f"{name}: pixel_count"
    e_max = (wmax.double() - want["max"]).abs()
    e_sum = (wsum.double() - want["sum"]).abs()
    bar_sum = want["count"].double() * PAR.IMG_SHARP
    f_max = float(e_max.max() / PAR.IMG_SHARP)
    f_sum = float((e_sum[bar_sum > 0] / bar_sum[bar_sum > 0]).max())
    print(f"\n[importance] {name}: weight_max at most {f_max:.3f} of IMG_SHARP, weight_sum at most {f_sum:.3f} of "
          f"count x IMG_SHARP")
    assert bool((e_max <= PAR.IMG_SHARP).all()) and bool((e_sum <= bar_sum).all())
    assert bool((wsum[want["count"] == 0] == 0).all()) and bool((wmax[want["count"] == 0] == 0).all())


# ---- 3. identity with the alpha image ------------------------------------------------------------------------------
def _n_contrib(g):
    """the forward's per-pixel n_contrib, read from its image state (final_T, then n_contrib, each W H words padded
    to 256 bytes: csrc/capi.hip ImageState::carve); checked against the alpha image it sits behind"""
    s = g["sc"]["s"]
    N = int(s["W"]) * int(s["H"])
    ib = g["fwd"][6]
    assert ib.data_ptr() % 256 == 0
    off = (4 * N + 255) // 256 * 256
    final_T = ib[:4 * N].view(torch.float32)
    alpha = _C().alpha_image(ib, int(s["H"]), int(s["W"])).reshape(-1)
    assert torch.equal(1.0 - final_T, alpha)
    return ib[off:off + 4 * N].view(torch.int32), alpha


@pytest.mark.parametrize("name", ["opaque", "dense0", "stack"])
def test_sums_add_up_to_the_alpha_image(name):
    g = gpu(name)
    wsum, wmax, count = g["scores"]
    n_contrib, alpha = _n_contrib(g)
    total = float(alpha.double().sum())
    got = float(wsum.double().sum())
    Kmax, Nmax, pairs = int(n_contrib.max()), int(count.max()), int(count.long().sum())
    # the precondition of the bar's derivation (module docstring), from the GPU's own counts
    assert pairs / total <= (3 * Kmax - 2) / 2, (pairs, total, Kmax)
    bar = (3 * Kmax + Nmax) * U * total
    print(f"\n[importance] {name}: sum of weight_sum {got:.6f}, sum of the alpha image {total:.6f}, difference "
          f"{abs(got - total) / bar:.4f} of (3 Kmax + Nmax) u total (Kmax {Kmax}, Nmax {Nmax}, {pairs} blended pairs)")
    assert total > 100 and abs(got - total) <= bar


# ---- 4. structure ---------------------------------------------------------------------------------------------------
def test_a_scene_without_instances_gives_zeros():
    g = gpu("behind")
    assert g["fwd"][0] == 0 and len(g["sc"]["s"]["means3D"]) == 12
    wsum, wmax, count = g["scores"]
    assert wsum.dtype == torch.float32 and wmax.dtype == torch.float32 and count.dtype == torch.int32
    assert tuple(wsum.shape) == tuple(wmax.shape) == tuple(count.shape) == (12,)
    assert not bool(wsum.any()) and not bool(wmax.any()) and not bool(count.any())


def test_culled_gaussians_give_exact_zeros():
    """`sparse` with two Gaussians behind the camera (radii == 0) and three too faint to reach 1/255 anywhere (radii > 0,
    no instance survives the exact culling); in `sparse` itself whatever has no instance"""
    for name in ("sparse_culled", "sparse"):
        g = gpu(name)
        wsum, wmax, count = g["scores"]
        out = _C().debug_tile_lists(g["fwd"][4], g["fwd"][5], g["fwd"][6], 12, 70, 45, g["fwd"][0])
        listed = torch.zeros(12, dtype=torch.bool, device="cuda:0")
        listed[out[3].long()] = True
        for t in (wsum, wmax, count):
            assert not bool(t[~listed].any()), name
        assert bool((count[listed] > 0).any())
        if name == "sparse_culled":
            radii = g["fwd"][3]
            assert not bool(radii[IR.SPARSE_BEHIND].any()) and bool((radii[IR.SPARSE_FAINT] > 0).all())
            assert not bool(listed[IR.SPARSE_BEHIND + IR.SPARSE_FAINT].any()) and int(listed.sum()) == 7
            _check_onehot(name, range(12))


def test_a_gaussian_whose_slots_span_three_waves():
    g = gpu("wide")
    s = g["sc"]["s"]
    out = _C().debug_tile_lists(g["fwd"][4], g["fwd"][5], g["fwd"][6], 21, 256, 256, g["fwd"][0])
    gid, slot = out[3].cpu().numpy(), out[5].cpu().numpy()
    mine = np.sort(slot[gid == IR.WIDE_BIG])
    assert len(mine) > 128 and np.array_equal(mine, np.arange(mine[0], mine[0] + len(mine)))  # consecutive slots
    waves = mine[-1] // 64 - mine[0] // 64 + 1
    assert waves >= 3
    ref, used = _check_onehot("wide", range(21))
    k = ref["ids"].index(IR.WIDE_BIG)
    print(f"\n[importance] wide: Gaussian {IR.WIDE_BIG} has {len(mine)} slots over {waves} waves, reaches "
          f"{int(ref['count'][k])} pixels; sum error at most {used:.3f} of n u S")
    assert int(ref["count"][k]) > 128 * 64


# ---- 5. repeatable and inert ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense0", "opaque", "stack"])
def test_two_calls_give_the_same_bits_and_change_nothing(name):
    g = gpu(name)
    sc, fwd = g["sc"], g["fwd"]
    before = [t.clone() for t in fwd[1:]]
    a = _importance(sc, fwd)
    b = _importance(sc, fwd)
    for x, y, z in zip(a, b, g["scores"]):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y in zip(before, fwd[1:]):  # colour, depth, radii and the three state buffers
        assert torch.equal(x, y)


def test_a_backward_after_the_pass_is_the_backward_without_it():
    from gpu_helpers import c_backward
    sc = _scene("dense0")
    s = sc["s"]
    d = to_dev(s, torch.device("cuda:0"))
    grad = torch.tensor(np.random.default_rng(5).normal(0, 1, (3, s["H"], s["W"])).astype(np.float32), device="cuda:0")
    plain = _forward(sc, d, None, None)
    want = c_backward(_C(), s, d, plain, grad)
    fwd = _forward(sc, d, None, None)
    _importance(sc, fwd)
    got = c_backward(_C(), s, d, fwd, grad)
    for n, x, y in zip(PAR.GRAD_NAMES, got, want):
        assert torch.equal(x, y), n
    assert float(want[3].abs().max()) > 0


# ---- 6. antialiasing ------------------------------------------------------------------------------------------------
def test_antialiased_scores_are_the_antialiased_forwards():
    P = len(_scene("small0")["s"]["means3D"])
    ref, used = _check_onehot("small0", range(P), aa=True)
    plain, anti = gpu("small0")["scores"], gpu("small0", aa=True)["scores"]
    assert not torch.equal(plain[0], anti[0]) and not torch.equal(plain[1], anti[1])
    print(f"\n[importance] small0 antialiased: sum error at most {used:.3f} of n u S; largest max "
          f"{float(anti[1].max()):.4f} against {float(plain[1].max()):.4f} plain")


# ---- 7. stream ------------------------------------------------------------------------------------------------------
def test_the_pass_on_a_side_stream():
    """tests/test_streams_gpu.py's pattern, through its harness (stream_cases.run_case) with a case of this file's own:
    the forward and the pass queued on a side stream behind delayed copies of the inputs, with the null stream
    blocked, give the default stream's bits.  A launch, memset or copy of the pass that went to the null stream would
    run after the result was read."""
    import stream_cases as SC

    def call(t):
        fwd = SC.raster_forward(t)  # queued on the same stream just before the pass
        return list(_C().gaussian_importance(fwd[4], fwd[5], fwd[6], fwd[0], SC.RASTER["P"], SC.RASTER["H"],
                                             SC.RASTER["W"]))
    case = SC.Case("gaussian_importance", ["gaussian_importance"], SC.raster_inputs, call)
    cal = SC.calibration("cuda:0")
    host, want = SC.run_case(case, cal.fresh_stream())
    assert len(host) == 3 and float(host[0].sum()) > 0 and int(host[2].sum()) > 0


# ---- 8. upper layers ------------------------------------------------------------------------------------------------
def _model_and_views():
    """gs4d_train.synthetic's small 4D scene (bouncing_balls, 3 x 200 points at t = 0) as a GaussianModel with its
    optimizer, the deformation network re-drawn so that the timestamps differ, and three cameras at two timestamps"""
    if "model" not in _GPU:
        from gs4d_train import config
        from gs4d_train.gaussians import GaussianModel
        from gs4d_train.synthetic import SH_C0, bouncing_balls, look_at_camera
        hyper, opt = config.dynerf()
        canon, means_at = bouncing_balls(n_per_ball=200, seed=3)
        cols = np.clip(canon["shs"][:, 0, :] * SH_C0 + 0.5, 0, 1).astype(np.float32)
        torch.manual_seed(11)
        g = GaussianModel(3, hyper, fused=True)
        g.create_from_pcd(means_at(0.0), cols, 1.0)
        net = g._deformation.deformation_net
        net.grid.fused = True
        net.fused_heads = True
        with torch.no_grad():
            for level in net.grid.grids:
                for p in level:
                    p.copy_(torch.rand_like(p) * 0.4 + 0.1)
            for m in net.modules():
                if isinstance(m, torch.nn.Linear):
                    m.weight.copy_(torch.randn_like(m.weight) / m.in_features ** 0.5)
                    m.bias.copy_(0.02 * torch.randn_like(m.bias))
        g.training_setup(opt)
        g.active_sh_degree = 3
        cams = [look_at_camera(64, 48, (4.0 * math.sin(0.4 * i), 0.3, -4.0 * math.cos(0.4 * i)), time=(0.0, 0.5, 0.5)[i])
                for i in range(3)]
        _GPU["model"] = (g, cams, hyper, opt)
    return _GPU["model"]


def test_infer_importance_accumulates_the_views():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import infer
    g, cams, _, _ = _model_and_views()
    state = infer.prepare(g)
    got = infer.importance(state, cams)
    again = infer.importance(state, cams)
    P = g.get_xyz.shape[0]
    assert set(got) == {"sum", "max", "count", "views"}
    assert [got[k].dtype for k in ("sum", "max", "count", "views")] == [torch.float64, torch.float32, torch.int64,
                                                                        torch.int64]
    for k in got:
        assert tuple(got[k].shape) == (P,) and torch.equal(got[k], again[k]), k
    tot = torch.zeros(P, dtype=torch.float64, device="cuda")
    top = torch.zeros(P, device="cuda")
    cnt = torch.zeros(P, dtype=torch.int64, device="cuda")
    views = torch.zeros(P, dtype=torch.int64, device="cuda")
    per_view = []
    for cam in cams:
        st = infer._raster_settings(cam, state, torch.zeros(3, device="cuda"))
        m3, sc, rot, op, sh = infer.state_at_time(state, cam.time)
        ws, wm, c, radii = dgr.gaussian_importance(m3, op, shs=sh, scales=sc, rotations=rot, raster_settings=st)
        tot += ws.double()
        top = torch.maximum(top, wm)
        cnt += c.long()
        views += (radii > 0).long()
        per_view.append(ws)
    assert torch.equal(got["sum"], tot) and torch.equal(got["max"], top) and torch.equal(got["count"], cnt)
    assert torch.equal(got["views"], views) and int(views.max()) == 3 and float(tot.sum()) > 100
    assert not torch.equal(per_view[0], per_view[1])  # another camera, another time
    # the model is untouched: no graph, no gradient
    assert all(p.grad is None for p in (g._xyz, g._opacity))


def test_prune_by_importance_keeps_the_better_half():
    from gs4d_train import pruning, surgery
    from gs4d_train.synthetic import make_training_views
    from gs4d_train.train import train_step
    g, cams, hyper, opt = _model_and_views()
    bg = torch.ones(3, device="cuda")
    views = make_training_views(2, 64, 48, seed=6)
    train_step(g, views, opt, hyper, 3001, bg)  # the Adam moments are no longer zero
    P = g.get_xyz.shape[0]
    groups = {gr["name"]: gr for gr in g.optimizer.param_groups if gr["name"] in surgery.PARAMS}
    snap = {}
    for name, gr in groups.items():
        p = gr["params"][0]
        st = g.optimizer.state[p]
        snap[name] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        assert float(st["exp_avg"].abs().max()) > 0, name
    n_removed, scores = pruning.prune_by_importance(g, cams, keep_fraction=0.5)
    assert n_removed == P - math.ceil(P / 2) and g.get_xyz.shape[0] == math.ceil(P / 2)
    keep = (~pruning.importance_mask(scores, keep_fraction=0.5)).nonzero().squeeze(1)
    assert float(scores["sum"][keep].min()) >= float(scores["sum"][pruning.importance_mask(scores, keep_fraction=0.5)].max())
    for gr in g.optimizer.param_groups:
        if gr["name"] not in snap:
            continue
        p = gr["params"][0]
        st = g.optimizer.state[p]
        p0, m0, v0 = snap[gr["name"]]
        assert torch.equal(p.detach(), p0[keep]), gr["name"]
        assert torch.equal(st["exp_avg"], m0[keep]) and torch.equal(st["exp_avg_sq"], v0[keep]), gr["name"]
    assert g.max_radii2D.shape[0] == g.xyz_gradient_accum.shape[0] == g.denom.shape[0] == math.ceil(P / 2)
    loss = train_step(g, views, opt, hyper, 3002, bg)
    assert math.isfinite(float(loss))
    with pytest.raises(ValueError):
        pruning.prune_by_importance(g, cams)
    _GPU.pop("model")  # pruned: the next user builds a fresh one


def test_radsplat_rule_changes_the_render_by_what_it_removes():
    """Gaussians whose largest weight is below 0.01 are removed from `opaque` drawn with colours in [0, 1] over a
    background in [0, 1].  Removing, back to front, the removed Gaussians a pixel blends changes its colour by
    w_j (B_j - c_j) each -- B_j the colour of everything behind j, in [0, 1] like c_j, and w_j the ORIGINAL weight,
    which removals behind j do not touch -- so by less than 0.01 per removed Gaussian of the pixel's tile list."""
    from gs4d_train.pruning import importance_mask
    sc = AS.scene("opaque")
    s = sc["s"]
    P, H, W = len(s["means3D"]), int(s["H"]), int(s["W"])
    dev = torch.device("cuda:0")
    d = to_dev(s, dev)
    rng = np.random.default_rng(17)
    colors = torch.tensor(rng.uniform(0, 1, (P, 3)).astype(np.float32), device=dev)
    d["bg"] = torch.tensor([0.2, 0.5, 0.9], device=dev)
    draw = dict(s=s, use_sh=False)
    fwd = _forward(draw, d, colors, None)
    wsum, wmax, count = _importance(draw, fwd)
    scores = {"sum": wsum.double(), "max": wmax, "count": count.long()}
    mask = importance_mask(scores, min_max_weight=0.01)
    assert 0 < int(mask.sum()) < P and bool((wmax[mask] < 0.01).all()) and bool((wmax[~mask] >= 0.01).all())
    assert bool((count[mask] > 0).any())  # something that was drawn goes
    keep = ~mask
    d2 = dict(d)
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        d2[k] = d[k][keep].contiguous()
    after = _forward(draw, d2, colors[keep].contiguous(), None)
    # removed Gaussians in each tile's list, from the first forward's lists
    out = _C().debug_tile_lists(fwd[4], fwd[5], fwd[6], P, W, H, fwd[0])
    ranges, gid = out[0].cpu().numpy().astype(np.int64), out[3].cpu().numpy().astype(np.int64)
    removed = mask.cpu().numpy()
    per_tile = np.array([int(removed[gid[a:b]].sum()) for a, b in ranges])
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    per_pixel = torch.tensor(per_tile[(ys // 16) * gx + xs // 16], device=dev)
    diff = (after[1] - fwd[1]).abs().max(0).values
    bar = per_pixel.double() * 0.01
    worst = float((diff.double()[bar > 0] / bar[bar > 0]).max())
    print(f"\n[importance] opaque, max < 0.01: {int(mask.sum())} of {P} removed, up to {int(per_pixel.max())} in a "
          f"tile; the render moves by at most {float(diff.max()):.5f}, {worst:.3f} of count x 0.01")
    assert bool((diff.double() <= bar).all())
