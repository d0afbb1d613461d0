"""Every route of gs4d_train/deformation.py's dispatch, end to end through the module, against the fp64 unfused graph.

tests/test_train_gpu.py checks each gs4d_train._C entry of the deformation MLP by hand; this file checks the wiring
between them -- which gradient lands in which slot, the column slices, the ReLU mask through h, the split of the
packed first layers' gradient, the zero fill of an unused output -- on one scene per leaf of the dispatch rule
(tests/deformation_route_scenes.py; its CPU preconditions are tests/test_deformation_routes_boundary.py).

Route: counters around the _C entries equal the rule's restatement (expected_calls) exactly.
Value, fp32: for every tensor T (each active head's output, every parameter gradient, the points' gradient), with
e = max |T - T64| / max |T64|, the fused run's e_f <= max(4 e_u, 1e-6), e_u the fp32 unfused graph's on the same
GPU: 4 for another order of the same number of fp32 additions, 1e-6 (eight fp32 ulps of the largest element) so that
a tensor both get right to the last bit cannot fail on one ulp.  TERMS_BARRED lists the tensors held to the kernel
tests' elementwise 1e-5 of the |terms| sum instead, each with the reason.
Value, bf16: 5 % relative L2 of the fp64 result per tensor (test_train_step_bf16_mlp_tracks_fp32's bar): a wrong slot
moves a tensor by its whole norm; the sharp bf16 bounds are the kernel tests'."""
import functools

import pytest
import torch

import deformation_route_scenes as S

pytestmark = pytest.mark.gpu

# (scene, tensor): why its error exceeds 4 e_u though the kernel is right -- none needed so far
TERMS_BARRED = {}


class _Counters:
    """counters around the MLP entries of gs4d_train._C, as test_shape_48_128_gpu._count_calls"""

    def __init__(self, monkeypatch):
        from gs4d_train import _C
        self.calls = dict.fromkeys(S.ENTRIES, 0)
        for name in S.ENTRIES:
            if ":" not in name:
                monkeypatch.setattr(_C, name, self._counted(name, getattr(_C, name)))

    def _counted(self, name, real):
        def counted(*a, **k):
            self.calls[name] += 1
            if k.get("with_hb", False):
                self.calls[name + ":with_hb"] += 1
            return real(*a, **k)
        return counted

    def snapshot(self):
        return dict(self.calls)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """One fused run under counters, then the fp32 and fp64 unfused graphs on the same GPU, once per scene:
    (net, fused tensors, fp32 unfused tensors, fp64 tensors, the fused run's calls, the calls the references added)"""
    s = S.SCENES[name]
    with pytest.MonkeyPatch.context() as mp:
        counters = _Counters(mp)
        net = S.build(s, "cuda", fused=True)
        of, gf = S.run(net, s)
        fused_calls = counters.snapshot()
        o32, g32 = S.run(S.reference_net(net, torch.float32), s)
        o64, g64 = S.run(S.reference_net(net), s, torch.float64)
        after = counters.snapshot()
    torch.cuda.synchronize()
    added = {k: after[k] - fused_calls[k] for k in after}
    return net, {**of, **gf}, {**o32, **g32}, {**o64, **g64}, fused_calls, added


@pytest.mark.parametrize("name", list(S.SCENES))
def test_route_is_the_restated_one(name):
    s = S.SCENES[name]
    net, _, _, _, calls, added = _scene(name)
    assert net.grid.feat_dim == s.feat_dim and net.W == s.W and len(net.feature_out) == 2 * max(s.depth, 1) - 1
    want = S.expected_calls(s.feat_dim, s.W, s.depth, [S.HEAD_N[i] for i in s.heads], s.dtype, s.P)
    print(f"\n[routes] {name}: " + ", ".join(f"{k} {v}" for k, v in calls.items() if v) + ("" if any(calls.values()) else "no _C MLP call"))
    assert calls == want, {k: (calls[k], want[k]) for k in want if calls[k] != want[k]}
    assert not any(added.values()), f"the unfused references called {added}"


@pytest.mark.parametrize("name", S.FP32)
def test_fp32_values_match_fp64_as_closely_as_the_unfused_graph(name):
    s = S.SCENES[name]
    net, got, control, want, _, _ = _scene(name)
    assert all(S.HEADS[i] in want for i in s.heads) and "xyz" in want and "grid.grids.0.0" in want
    for i in s.loss:  # each first- and second-layer weight and bias of the heads the loss reads, separately
        assert all(f"{S.HEADS[i]}.{j}.{w}" in want for j in (1, 3) for w in ("weight", "bias"))
    terms = {k: t for k, t in S.sum_terms(net, s).items() if (name, k) in TERMS_BARRED}
    figures, failures = S.compare(got, control, want, terms, S.flipped_rows(net, s))
    cls = {}
    for k, (e_f, e_u) in figures.items():
        c = ("output" if k in S.HEADS else "xyz" if k == "xyz" else "planes" if k.startswith("grid") else
             "feature_out" if k.startswith("feature_out") else "heads' first layers" if ".1." in k else
             "heads' second layers")
        cls[c] = tuple(map(max, zip(cls.get(c, (0.0, 0.0)), (e_f, e_u))))
    print(f"\n[routes] {name}: " + "; ".join(f"{c} e_f {a:.1e} e_u {b:.1e}" for c, (a, b) in cls.items()))
    assert not failures, "\n".join(failures)
    # the tensors the fused run has beyond the reference's are the zero fill of outputs the loss does not read
    extra = set(got) - set(want)
    assert extra == {f"{S.HEADS[i]}.{j}.{w}" for i in s.heads if i not in s.loss for j in (1, 3) for w in ("weight", "bias")}


@pytest.mark.parametrize("name", S.BF16)
def test_bf16_values_stay_within_the_bf16_bar(name):
    net, got, _, want, _, _ = _scene(name)
    assert set(got) == set(want)
    worst = ("", 0.0)
    for k in want:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        rel = S.rel_l2(got[k], want[k])
        worst = max(worst, (k, rel), key=lambda kv: kv[1])
    print(f"\n[routes] {name}: largest relative L2 error {worst[1]:.2e} ({worst[0]}), bar 5e-2")
    for k in want:
        assert S.rel_l2(got[k], want[k]) <= 5e-2, (k, S.rel_l2(got[k], want[k]))


@pytest.mark.parametrize("name", list(S.SCENES))
def test_fresh_identically_seeded_model_gives_the_same_bits(name):
    s = S.SCENES[name]
    _, got, _, _, _, _ = _scene(name)
    o2, g2 = S.run(S.build(s, "cuda", fused=True), s)
    again = {**o2, **g2}
    assert set(again) == set(got)
    assert all(torch.equal(again[k], got[k]) for k in got), [k for k in got if not torch.equal(again[k], got[k])]


@pytest.mark.parametrize("name", ["dynerf", "skip_opacity"])
def test_second_backward_accumulates_exactly(name):
    """two passes without zero_grad: every .grad is bitwise twice the single pass's (x + x is exact), through the
    views _Stacked's backward hands the separate first-layer parameters"""
    s = S.SCENES[name]
    _, got, _, _, _, _ = _scene(name)
    net = S.build(s, "cuda", fused=True)
    S.run(net, s)
    _, twice = S.run(net, s, zero=False)
    for k in got:
        if k not in S.HEADS and k != "xyz":  # the points are a fresh leaf per pass
            assert torch.equal(twice[k], got[k] + got[k]), k
    assert torch.equal(twice["xyz"], got["xyz"])


@pytest.mark.parametrize("name", ["dynerf", "skip_opacity"])
def test_repacked_first_layers_give_the_same_bits(name):
    """one head parameter moved to storage of its own: the next step packs the first layers again and computes the
    first step's bits; the parameters stay the same objects with the same values"""
    from gs4d_train.deformation import _stacked
    s = S.SCENES[name]
    _, got, _, _, _, _ = _scene(name)
    net = S.build(s, "cuda", fused=True)
    heads = [getattr(net, S.HEADS[i]) for i in s.heads]
    S.run(net, s)
    assert _stacked([hd[1].weight for hd in heads]) is not None and _stacked([hd[1].bias for hd in heads]) is not None
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    ids = {n: id(p) for n, p in net.named_parameters()}
    moved = heads[1][1]
    moved.weight.data = moved.weight.data.clone()
    moved.bias.data = moved.bias.data.clone()
    assert _stacked([hd[1].weight for hd in heads]) is None and _stacked([hd[1].bias for hd in heads]) is None
    o2, g2 = S.run(net, s)
    again = {**o2, **g2}
    assert all(torch.equal(again[k], got[k]) for k in got), [k for k in got if not torch.equal(again[k], got[k])]
    ws = [hd[1].weight for hd in heads]
    assert all(a.data_ptr() + a.numel() * 4 == b.data_ptr() for a, b in zip(ws, ws[1:])), "not packed again"
    assert all(id(p) == ids[n] and torch.equal(p, before[n]) for n, p in net.named_parameters())


@pytest.mark.parametrize("name", ["dynerf", "default"])
def test_no_grad_forward_agrees_and_calls_no_mlp_kernel(name, monkeypatch):
    s = S.SCENES[name]
    net, got, control, want, _, _ = _scene(name)
    counters = _Counters(monkeypatch)
    ins, _, time = S.inputs(s, "cuda")
    with torch.no_grad():
        outs = net(*ins, time)
    assert not any(counters.calls.values()), counters.calls
    plain = {S.HEADS[i]: outs[i] for i in s.heads}
    heads = {k: want[k] for k in plain}
    figures, failures = S.compare(plain, control, heads)
    assert not failures, "\n".join(failures)
    for k in plain:  # and with the training forward: both within the bar of the same fp64 values
        d = float((plain[k] - got[k]).abs().max()) / float(want[k].abs().max())
        assert d <= max(S.FACTOR * figures[k][1], S.FLOOR) + max(S.FACTOR * figures[k][1], S.FLOOR), (k, d)
