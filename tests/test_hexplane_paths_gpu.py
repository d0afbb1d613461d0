"""The HexPlane field's backward, route by route, against exact references (scenes, the route classifier and the
references: tests/hexplane_path_scenes.py; their CPU preconditions: tests/test_hexplane_paths_boundary.py).

Exact scenes    every term is exactly representable and the sums are integer, so features, point gradients and plane
                gradients equal the fp64 grid_sample graph as floats, element for element (-0 counts as 0), through
                the LDS window, every feature slice, the direct atomics, under any point order and twice in a row.
Scaling         dfeat times 2^-100 and 2^100 scales the gradients by exactly that (hex_plane_scale's clamp at 2^127
                and its negative exponents).
General values  the same workgroups with uniform planes, points inside each workgroup's box and randn dfeat, under
                test_hexplane_small_distinct_planes' bars.
Morton order    the returned order against a stable argsort of a numpy restatement of the codes.
Tall planes     anchors at rows >= 32768 (bit 31 of y0 << 16 | x0).
Regulariser     edge shapes of the fused HexPlane regularisers against compute_regulation's arithmetic in fp64.
"""
import numpy as np
import pytest
import torch

import hexplane_path_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device(s):
    pts = torch.tensor(s["pts"], device=DEV)
    planes = [torch.tensor(p, device=DEV) for p in s["planes"]]
    return pts, planes, torch.tensor(s["dfeat"], device=DEV)


def _order(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)


def _assert_same(got, want, what):
    """got (fp32, device) equals want (fp64 reference, or an fp32 tensor) as floats, element for element"""
    got = got.detach().cpu()
    want = want.detach().cpu()
    want = want.float() if want.dtype == torch.float64 else want
    assert got.shape == want.shape and got.dtype == torch.float32, what
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


def _backward_checks(name, s, ref, both_entries=True):
    from gs4d_train import _C
    from gs4d_train.kernels import hexplane
    f64, d64, g64 = ref
    pts, planes, dfeat = _device(s)
    N = len(s["pts"])
    if both_entries:  # kernels.hexplane under autograd (the library's own, possibly kept, order)
        p = pts.clone().requires_grad_(True)
        pl = [x.clone().requires_grad_(True) for x in planes]
        feat = hexplane(p, [pl[i:i + 6] for i in range(0, len(pl), 6)])
        got = torch.autograd.grad(feat, [p] + pl, dfeat)
        _assert_same(feat, f64, name + " autograd feat")
        _assert_same(got[0], d64, name + " autograd dpts")
        for k, (a, b) in enumerate(zip(got[1:], g64)):
            _assert_same(a, b, "%s autograd plane %d" % (name, k))
    # _C with the scene's order: the workgroups the classifier saw
    feat, packed, order = _C.hexplane_forward(pts, planes, _order(s["order"]))
    assert torch.equal(order.cpu(), torch.tensor(s["order"], dtype=torch.int32))
    _assert_same(feat, f64, name + " feat")
    d0, g0 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    _assert_same(d0, d64, name + " dpts")
    for k, (a, b) in enumerate(zip(g0, g64)):
        _assert_same(a, b, "%s plane %d (level %d, plane %d)" % (name, k, k // 6, k % 6))
    d1, g1 = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    assert torch.equal(d0, d1) and all(torch.equal(a, b) for a, b in zip(g0, g1)), name + ": second backward"
    return pts, planes, dfeat, packed, d0, g0


@pytest.mark.parametrize("name", S.EXACT)
def test_exact_scene_every_route_bitwise(name):
    """Features, dpts and every plane gradient equal the fp64 graph, through kernels.hexplane under autograd and
    through _C.hexplane_backward with the scene's order (whose routes the boundary test lists); a second backward
    gives the same bits; so do a random permutation and the library's own Morton order -- the sums are exact, so
    the grouping must not matter."""
    from gs4d_train import _C
    s = S.scene(name)
    pts, planes, dfeat, packed, d0, g0 = _backward_checks(name, s, S.reference64(name))
    N = len(s["pts"])
    perm = np.random.default_rng(5).permutation(N)
    feat_m, _, morton = _C.hexplane_forward(pts, planes)
    assert sorted(morton.cpu().tolist()) == list(range(N))
    for what, order in (("permuted", _order(perm)), ("Morton", morton)):
        feat, _, _ = _C.hexplane_forward(pts, planes, order)
        _assert_same(feat, S.reference64(name)[0], "%s %s feat" % (name, what))
        d, g = _C.hexplane_backward(pts, planes, packed, dfeat, order)
        _assert_same(d, d0, "%s %s dpts" % (name, what))
        for k, (a, b) in enumerate(zip(g, g0)):
            _assert_same(a, b, "%s %s plane %d" % (name, what, k))
    _assert_same(feat_m, S.reference64(name)[0], name + " Morton feat")
    if name == "zero_plane":
        assert [bool(x.any()) for x in g0] == [k == s["zero_plane"] for k in range(12)]


@pytest.mark.parametrize("name", S.EXACT)
def test_exact_scene_power_of_two_scaling(name):
    """dfeat * 2^-100 and dfeat * 2^100 (both exact): the plane gradients and dpts are the fp64 results times that
    power, element for element.  2^-100 drives hex_plane_scale's exponent into its clamp at 127 (the conversion then
    multiplies by 2^-127), 2^100 makes it negative."""
    from gs4d_train import _C
    s = S.scene(name)
    _, d64, g64 = S.reference64(name)
    pts, planes, dfeat = _device(s)
    _, packed, order = _C.hexplane_forward(pts, planes, _order(s["order"]))
    for e in (-100, 100):
        k = 2.0 ** e
        d, g = _C.hexplane_backward(pts, planes, packed, dfeat * k, order)
        _assert_same(d, d64 * k, "%s dpts at 2^%d" % (name, e))
        for i, (a, b) in enumerate(zip(g, g64)):
            assert torch.equal((b * k).float().double(), b * k)  # still a float
            _assert_same(a, b * k, "%s plane %d at 2^%d" % (name, i, e))


WORST = {}


@pytest.mark.parametrize("name", S.EXACT)
def test_general_values_within_the_field_bars(name):
    """The scene's workgroups with uniform plane values in [0.1, 1.2], points uniform inside each workgroup's box and
    randn dfeat, against the fp64 graph under test_hexplane_small_distinct_planes' bars: features rtol 1e-5 /
    atol 1e-6, dpts and every plane gradient to 1e-4 of the tensor's maximum.  Prints the worst ratios to the bars.
    The points lie on a 2^-20 lattice, where fp32 unnormalises a coordinate exactly on these 2^k + 1 axes
    (hexplane_path_scenes.general): off it, on the 2049-node and 32769-node axes, fp32's coordinate rounding alone
    exceeds the feature bar, in the fp32 torch graph exactly as in the kernel (12x and 318x, measured).
    Measured on the MI355X, worst over the scenes: features 0.031, dpts 0.0034, plane gradients 0.0027 of their bars."""
    from gs4d_train import _C
    s = S.general(name)
    f64, d64, g64 = S.reference64(name, "general")
    pts, planes, dfeat = _device(s)
    feat, packed, order = _C.hexplane_forward(pts, planes, _order(s["order"]))
    d, g = _C.hexplane_backward(pts, planes, packed, dfeat, order)
    rf = float(((feat.cpu().double() - f64).abs() / (1e-6 + 1e-5 * f64.abs())).max())
    rb = []
    for a, b in zip([d] + list(g), [d64] + g64):
        assert bool(torch.isfinite(a).all())
        rb.append(float((a.cpu().double() - b).abs().max()) / (1e-4 * max(float(b.abs().max()), 1e-30)))
    WORST[name] = (rf, rb[0], max(rb[1:]))
    print("hexplane general %-12s worst / bar: feat %.4f dpts %.5f planes %.5f" % ((name,) + WORST[name]))
    assert rf <= 1.0 and max(rb) <= 1.0, (name, rf, rb)


@pytest.mark.parametrize("name", ["tall_exact", S.TALL_40000])
def test_tall_time_plane_rows_past_32767(name):
    """A (1, 4, H, 3) time plane with anchors at rows 32767, 32768 and beyond: the anchor packs as y0 << 16 | x0, which
    a signed word took for "no anchor" from row 32768 on, dropping the points' terms without a trace.  tall_exact
    (H = 32769) is compared element for element like every exact scene; the 40000-row plane, with anchors at rows
    32767, 32768 and 39998, cannot be made exact (hexplane_path_scenes.tall_scene: 39999 is odd) and is compared
    under the general-value bars, which the scene's row coordinates leave room for (asserted on the CPU).  In both
    the rows past 32767 must carry gradient."""
    s = S.scene(name)
    ref = S.reference64(name) if name == "tall_exact" else S.torch_graph(s, torch.float64)
    if name == "tall_exact":
        g2 = _backward_checks(name, s, ref)[5][2]
    else:
        from gs4d_train import _C
        pts, planes, dfeat = _device(s)
        feat, packed, order = _C.hexplane_forward(pts, planes, _order(s["order"]))
        d, g = _C.hexplane_backward(pts, planes, packed, dfeat, order)
        torch.testing.assert_close(feat.cpu(), ref[0].float(), rtol=1e-5, atol=1e-6)
        ratios = []
        for a, b in zip([d] + list(g), [ref[1]] + ref[2]):
            ratios.append(float((a.cpu().double() - b).abs().max()) / (1e-4 * float(b.abs().max())))
        print("hexplane tall_40000 worst / bar: dpts %.5f planes %.5f" % (ratios[0], max(ratios[1:])))
        assert max(ratios) <= 1.0, ratios
        g2 = g[2]
    want = ref[2][2]
    for r in s["rows"]:
        assert bool(want[0, :, r].any()) and bool(g2[0, :, r].any()), r


@pytest.mark.parametrize("N", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_morton_order_is_a_stable_sort_of_the_codes(N):
    """_C.hexplane_forward's own order equals np.argsort(codes, kind="stable") of the numpy restatement of quant8 /
    spread3, for point counts around the code kernel's workgroup (256) and the sort's chunk (4096), with coordinates
    spread beyond [-1, 1] (clamped codes, many ties); a cloud of identical points keeps the identity order."""
    from gs4d_train import _C
    rng = np.random.default_rng(N)
    pts = rng.uniform(-1.3, 1.3, (N, 4)).astype(np.float32)
    pts[::7, :3] = np.round(pts[::7, :3] * 4) / 4  # code boundaries and ties
    planes = [torch.full((1, 4, 3, 3), 0.5, device=DEV) for _ in range(6)]
    _, _, order = _C.hexplane_forward(torch.tensor(pts, device=DEV), planes)
    assert np.array_equal(order.cpu().numpy().astype(np.int64), S.morton_order(pts))
    same = np.tile(pts[:1], (N, 1))
    _, _, order = _C.hexplane_forward(torch.tensor(same, device=DEV), planes)
    assert np.array_equal(order.cpu().numpy(), np.arange(N))


# ---- the regularisers' edge shapes ----------------------------------------------------------------------------------
def _reg_planes(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (C, H, W) in enumerate(shapes):
        t = 1.0 + 0.05 * (torch.rand(1, C, H, W, generator=g) - 0.5)
        t.view(-1)[::3] = 1.0  # exact ones: |1 - t|'s subgradient is 0
        out.append(t)
    return out


REG_CASES = {
    # name: ((C, H, W) per plane, weights (w_smooth, w_l1) per plane or None for the field's)
    "H3_W1_C1": ([(1, 3, 1)], [(1.0, 1e-4)]),  # one second-difference row, one element per row
    "H4_W2_C16": ([(16, 4, 2)], [(1.0, 1e-4)]),
    "H5_W7_C1": ([(1, 5, 7)], [(2e-4, 0.0)]),  # a spatial plane: no L1 term
    "H3_W7_C16": ([(16, 3, 7)], [(0.0, 1e-4)]),  # no smoothness term
    "n2047": ([(1, 23, 89)], [(1.0, 1e-4)]),  # one workgroup's share is 2048 elements
    "n2048": ([(16, 16, 8)], [(1.0, 1e-4)]),
    "n2049": ([(1, 3, 683)], [(1.0, 1e-4)]),
    "all_ones": ([(16, 5, 7)], [(1.0, 1e-4)]),
    "mixed24": ([(C, H, W) for C in (1, 16) for H in (3, 4, 5) for W in (1, 2, 7)] + [(1, 23, 89), (16, 16, 8),
                (1, 3, 683), (16, 4, 2), (1, 3, 1), (16, 5, 7)], None),
}


@pytest.mark.parametrize("case", list(REG_CASES))
def test_hexplane_regulation_edge_shapes(case):
    """The fused regularisers at H in {3, 4, 5}, W in {1, 2, 7}, C in {1, 16}, 2047 / 2048 / 2049 elements, 1 and 24
    planes (GS4D_REG_MAX_PLANES, four levels through kernels.hexplane_regulation and GaussianModel's
    compute_regulation), one of the two weights zero, and time planes of exact ones, against compute_regulation's
    arithmetic on fp64 copies under test_hexplane_regulation_fused_matches_torch's bars (loss 1e-5 relative, gradients
    1e-5 of the tensor's maximum); the value of the with_value pass is bitwise hexplane_regulation_value's (the
    forward's), its gradient bitwise the accumulate-only pass's, and a nonzero .grad is added to."""
    from types import SimpleNamespace

    from gs4d_train import _C
    from gs4d_train.gaussians import GaussianModel, compute_plane_smoothness
    shapes, weights = REG_CASES[case]
    planes = _reg_planes(shapes, len(case))
    if case == "all_ones":
        planes[0].fill_(1.0)
    scale = 2.5
    if weights is None:  # 24 planes as four levels of a field: time planes 2, 4, 5
        from gs4d_train.kernels import (hexplane_regulation, hexplane_regulation_accumulate_grad,
                                        hexplane_regulation_value)
        w = (1.0, 1e-4, 2e-4)  # time_smoothness_weight, l1_time_planes_weight, plane_tv_weight
        assert len(planes) == 24
        g64 = [[p.double().requires_grad_(True) for p in planes[i:i + 6]] for i in range(0, 24, 6)]
        m = GaussianModel.__new__(GaussianModel)
        m.fused = False
        m._deformation = SimpleNamespace(deformation_net=SimpleNamespace(grid=SimpleNamespace(grids=g64)))
        ref = m.compute_regulation(*w)
        flat64 = [p for l in g64 for p in l]

        def grids():
            return [[p.to(DEV).requires_grad_(True) for p in planes[i:i + 6]] for i in range(0, 24, 6)]
        gf = grids()
        lf = hexplane_regulation(gf, *w)
        (scale * lf).backward()
        auto = [p.grad for l in gf for p in l]
        ga, gb, gc = grids(), grids(), grids()
        pre = [torch.randn(p.shape, generator=torch.Generator().manual_seed(7)).to(DEV) for p in planes]
        for p, q in zip([p for l in gc for p in l], pre):
            p.grad = q.clone()
        v = hexplane_regulation_accumulate_grad(ga, *w, scale=scale, with_value=True)
        assert hexplane_regulation_accumulate_grad(gb, *w, scale=scale) is None
        hexplane_regulation_accumulate_grad(gc, *w, scale=scale)
        value = hexplane_regulation_value(ga, *w)
        with_value = [p.grad for l in ga for p in l]
        only = [p.grad for l in gb for p in l]
        added = [p.grad for l in gc for p in l]
    else:
        ws, wl = [a for a, _ in weights], [b for _, b in weights]
        flat64 = [p.double().requires_grad_(True) for p in planes]
        ref = sum(a * compute_plane_smoothness(p) + b * torch.abs(1 - p).mean() for p, a, b in zip(flat64, ws, wl))
        dev = [p.to(DEV) for p in planes]
        dloss = torch.full((1,), scale, device=DEV)
        lf = _C.hexplane_reg_forward(dev, ws, wl)
        auto = _C.hexplane_reg_backward(dev, ws, wl, dloss)
        pre = [torch.randn(p.shape, generator=torch.Generator().manual_seed(7)).to(DEV) for p in planes]
        with_value, only = [torch.zeros_like(p) for p in dev], [torch.zeros_like(p) for p in dev]
        added = [q.clone() for q in pre]
        v = _C.hexplane_reg_accumulate(dev, with_value, ws, wl, dloss, with_value=True)
        _C.hexplane_reg_accumulate(dev, only, ws, wl, dloss)
        _C.hexplane_reg_accumulate(dev, added, ws, wl, dloss)
        value = lf
    (scale * ref).backward()
    lf, ref_v = lf.detach(), float(ref.detach())
    assert abs(float(lf) - ref_v) <= 1e-5 * abs(ref_v), (float(lf), ref_v)
    assert torch.equal(v, value) and torch.equal(v, lf)
    for k, (p64, a, b, c, d, q) in enumerate(zip(flat64, auto, with_value, only, added, pre)):
        bar = 1e-5 * max(float(p64.grad.abs().max()), 1e-30)
        assert float((a.cpu().double() - p64.grad).abs().max()) <= bar, (case, k)
        assert torch.equal(b, c), (case, k)                      # with_value == accumulate-only, bitwise
        assert torch.equal(b, a), (case, k)                      # == the assigning backward (0 + g)
        assert torch.equal(d, q + c), (case, k)                  # added to what .grad held: one fp32 add
        assert bool((d != c).any())
    if case == "all_ones":
        assert float(lf) == 0.0 and not bool(auto[0].any())
