"""CPU preconditions of tests/test_deformation_routes_gpu.py: what its scenes (tests/deformation_route_scenes.py) must be
for the GPU comparisons to mean something.  The scenes reach every leaf of the restated dispatch rule; no ReLU input
of a scene sits close enough to zero for an fp32 evaluation to take the other side (which would move a whole row's term
of a weight gradient: the input's conditioning, not a kernel's error); the GPU tests' bar is one the plain fp32 torch
graph meets itself; and the comparison rejects a swapped and a short-changed gradient."""
import functools

import pytest
import torch

import deformation_route_scenes as S


@functools.lru_cache(maxsize=None)
def _cpu(name):
    """(net, fp64 outputs and gradients, fp32 unfused outputs and gradients) of a scene on the CPU"""
    s = S.SCENES[name]
    net = S.build(s)
    o64, g64 = S.run(S.reference_net(net), s, torch.float64)
    o32, g32 = S.run(S.reference_net(net, torch.float32), s)
    return net, {**o64, **g64}, {**o32, **g32}


def test_scene_table():
    """feat_dim, W, depth, heads and P of every scene; the field is the one small HexPlane"""
    rows = {n: (s.feat_dim, s.W, s.depth, len(s.heads), s.P) for n, s in S.SCENES.items()}
    assert rows == {
        "dnerf": (64, 64, 0, 3, 600), "dynerf": (32, 128, 0, 5, 600), "w64_five": (64, 64, 0, 5, 600),
        "default": (128, 64, 1, 3, 2500), "depth2": (32, 128, 2, 3, 600), "w256_three": (32, 256, 0, 3, 2500),
        "w256_even": (32, 256, 0, 3, 2400), "w256_five": (32, 256, 0, 5, 600), "w32": (32, 32, 0, 3, 600),
        "pos_only_loss": (32, 128, 0, 5, 600), "skip_opacity": (32, 128, 0, 4, 600), "rot_only": (32, 128, 0, 1, 600),
        "dynerf_p1": (32, 128, 0, 5, 1), "dynerf_p65": (32, 128, 0, 5, 65), "bf16_dynerf": (32, 128, 0, 5, 600),
        "bf16_dnerf": (64, 64, 0, 3, 2500), "bf16_w256": (32, 256, 0, 3, 2500), "bf16_default": (128, 64, 1, 3, 2500)}
    assert S.SCENES["pos_only_loss"].loss == (S.POS,) and S.SCENES["skip_opacity"].heads == (0, 1, 2, 4)
    assert all(s.loss == s.heads for n, s in S.SCENES.items() if n != "pos_only_loss")
    from gs4d_train import config
    d = config.model_hidden_params()
    assert (len(d.multires) * d.kplanes_config["output_coordinate_dim"], d.net_width, d.defor_depth) == (128, 64, 1), \
        "the `default` scene is no longer the library's default shape"
    h = S.hyper(S.SCENES["default"])
    assert h.kplanes_config["resolution"] == [8, 8, 8, 5] and (h.no_do, h.no_dshs, h.no_dx) == (True, True, False)


def test_scenes_reach_every_leaf_of_the_rule():
    reached = set()
    for name in S.SCENES:
        counts, leaves = S.scene_route(name)
        assert leaves <= set(S.LEAVES) and set(counts) == set(S.ENTRIES)
        reached |= leaves
    assert reached == set(S.LEAVES), sorted(set(S.LEAVES) - reached)


def test_fp32_scenes_differ_in_route_unless_stated():
    sig = {n: tuple(S.scene_route(n)[0][e] for e in S.ENTRIES) for n in S.FP32}
    for n in S.FP32:
        same = S.SCENES[n].same_as
        if same is None:
            twins = [m for m in S.FP32 if m != n and S.SCENES[m].same_as is None and sig[m] == sig[n]]
            assert not twins, (n, twins)
        else:
            assert same[0] in S.FP32 and S.SCENES[same[0]].same_as is None and same[1]
            assert sig[n] == sig[same[0]], (n, same[0])


def test_restated_counts_of_the_named_routes():
    """the counts of the routes DESIGN §10.2 names, as numbers"""
    z = dict.fromkeys(S.ENTRIES, 0)
    mfma = {**z, "feature_relu_forward": 1, "feature_relu_backward": 1, "heads_block_forward": 1, "heads_backward": 1,
            "mlp_dw_f32": 1, "mlp_dx_f32": 1}
    assert S.scene_route("dnerf")[0] == mfma and S.scene_route("dynerf")[0] == mfma
    assert S.scene_route("default")[0] == {**mfma, "feature_relu_forward": 0, "feature_relu_backward": 0}
    assert S.scene_route("w256_three")[0] == {**z, "heads_forward": 1, "heads_backward": 1, "gemm_f32": 3, "sum_slices": 1}
    assert S.scene_route("w256_even")[0] == {**z, "heads_forward": 1, "heads_backward": 1, "gemm_f32": 2, "sum_slices": 1}
    assert S.scene_route("w256_five")[0] == {**z, "heads_forward": 1, "linear_dw": 1, "gemm_f32": 2}
    assert S.scene_route("w32")[0] == {**z, "gemm_f32": 4}  # rocBLAS dW of three heads and the first layers; no MLP kernel
    assert S.scene_route("bf16_dynerf")[0] == {**z, "feature_relu_forward": 1, "feature_relu_forward:with_hb": 1,
                                               "feature_relu_backward": 1, "heads_block_forward_bf16": 1,
                                               "heads_backward": 1, "mlp_dw_bf16": 1, "mlp_dx_bf16": 1}
    assert S.scene_route("bf16_dnerf")[0] == {**z, "feature_relu_forward": 1, "feature_relu_forward:with_hb": 1,
                                              "feature_relu_backward": 1, "heads_block_forward_bf16": 1,
                                              "heads_backward": 1, "gemm_f32": 2, "sum_slices": 1, "mlp_dx_bf16": 1}
    assert S.scene_route("bf16_w256")[0] == z
    assert S.scene_route("bf16_default")[0] == {**z, "heads_block_forward_bf16": 1, "heads_backward": 1, "gemm_f32": 2,
                                                "sum_slices": 1, "mlp_dx_bf16": 1}


@pytest.mark.parametrize("name", S.FP32)
def test_committed_seed_has_no_relu_tie(name):
    """|z| of every ReLU input of the fp64 graph exceeds 8 x the measured fp32 rounding ratio x its |terms| sum"""
    s = S.SCENES[name]
    net = _cpu(name)[0]
    ratio = S.rounding_ratio(net, s)
    slack = S.tie_slack(net, s, ratio)
    print(f"\n[routes] {name}: seed {s.seed}, fp32 rounding {ratio:.2e} of the |terms| sum, smallest |z| / margin {slack:.2f}")
    assert 0 < ratio < 1e-6, "the fp32 torch graph no longer rounds like fp32"
    assert slack > 1.0
    assert not bool(S.flipped_rows(net, s).any())


@pytest.mark.parametrize("name", S.FP32)
def test_fp32_torch_graph_meets_the_gpu_bar(name):
    """The plain fp32 graph summed in another order (the rows reversed) against the plain fp32 graph as control: the
    bar e <= max(4 e_u, 1e-6) must let it through on every tensor, or it is no bar."""
    s = S.SCENES[name]
    net, want, control = _cpu(name)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in want.values())
    assert set(want) == set(control)
    perm = torch.arange(s.P - 1, -1, -1)
    o32, g32 = _run_permuted(S.reference_net(net, torch.float32), s, perm)
    figures, failures = S.compare({**o32, **g32}, control, want)
    worst = max(figures.items(), key=lambda kv: kv[1][0] / max(S.FACTOR * kv[1][1], S.FLOOR))
    print(f"\n[routes] {name}: fp32 torch reversed, closest to the bar {worst[0]} e {worst[1][0]:.2e} (e_u {worst[1][1]:.2e})")
    assert not failures, failures


def _run_permuted(net, s, perm):
    """S.run with the points in the order `perm`, the per-point results put back in the scene's order"""
    ins, ups, time = S.inputs(s)
    ins, ups = [t[perm].contiguous() for t in ins], [t[perm].contiguous() for t in ups]
    ins[0].requires_grad_(True)
    net.zero_grad(set_to_none=True)
    outs = net(*ins, time)
    sum((outs[i] * ups[i]).sum() for i in s.loss).backward()
    inv = torch.argsort(perm)
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    grads["xyz"] = ins[0].grad[inv]
    return {S.HEADS[i]: outs[i].detach()[inv] for i in s.heads}, grads


def test_comparison_rejects_swapped_and_short_gradients():
    s = S.SCENES["dynerf"]
    net, want, control = _cpu("dynerf")
    assert not S.compare(control, control, want)[1]
    a, b = "pos_deform.3.weight", "scales_deform.3.weight"
    assert control[a].shape == control[b].shape
    swapped = {**control, a: control[b], b: control[a]}
    failures = S.compare(swapped, control, want)[1]
    assert len(failures) == 2 and failures[0].startswith(a) and failures[1].startswith(b), failures
    # one row's term taken out of a weight gradient, for the second layers and for the packed first layers
    _, one = S.run(S.reference_net(net, torch.float32), s, rows=torch.tensor([s.P - 1]))
    for k in (a, "shs_deform.1.weight", "feature_out.0.weight"):
        assert float(one[k].abs().max()) > 0
        short = {**control, k: control[k] - one[k]}
        failures = S.compare(short, control, want, terms=S.sum_terms(net, s))[1]
        assert len(failures) == 1 and failures[0].startswith(k), (k, failures)
    # a missing tensor, a wrong shape, and a gradient where the reference has none
    assert S.compare({k: v for k, v in control.items() if k != a}, control, want)[1] == [a + ": missing"]
    assert len(S.compare({**control, a: control[a].t()}, control, want)[1]) == 1
    assert len(S.compare({**control, "extra": torch.ones(3)}, control, want)[1]) == 1
    assert not S.compare({**control, "extra": torch.zeros(3)}, control, want)[1]


def test_sum_terms_bound_the_reference_s_own_rounding():
    """the |terms| sums are those of the tensors they are named for: the fp32 graph lies within 1e-5 of them"""
    s = S.SCENES["dynerf"]
    net, want, control = _cpu("dynerf")
    terms = S.sum_terms(net, s)
    assert {k for k in want if k.endswith((".weight", ".bias"))} <= set(terms) and set(S.HEADS) <= set(terms)
    for k, t in terms.items():
        if k in want:
            assert t.shape == want[k].shape and bool((want[k].abs() <= t * (1 + 1e-12)).all()), k
            assert bool(((control[k].double() - want[k]).abs() <= S.TERMS_BAR * t).all()), k
