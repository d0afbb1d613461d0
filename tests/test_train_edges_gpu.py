"""Edge-case parity of the train-step tail kernels (deformation tail, densification statistics, one-launch Adam,
L1 loss, HexPlane field) against float64 restatements of their documented formulas (tests/train_edge_refs.py):
the shapes, branches and planted values at which these kernels can go wrong -- one row past a workgroup, P in
{0, 1}, every SH width, heads and upstream gradients that are absent, zero / tiny / huge quaternions, saturated
exp and sigmoid, more Adam tensors than one launch takes, the L1 total's fan-in edges, planes whose W != H.

Bars: c * 2^-24 * magnitude per element, c counted beside each bar in train_edge_refs.py (no bar comes from a
kernel's output; test_harness_cpu.py shows torch's own fp32 graphs inside the same bars); torch.equal where the
header promises exact results.  Every test prints the largest error it saw as a fraction of its bar."""
import pytest
import torch

import train_edge_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hold(section, got, ref, what, seen):
    """got within ref's bar (bitwise where the reference is exact); records the largest fraction of a bar used."""
    assert got.shape == ref.val.shape, (section, what, got.shape, ref.val.shape)
    if isinstance(ref.c, int) and ref.c == 0:
        assert torch.equal(got.double(), ref.val), (section, what, "exact")
        return
    w = R.worst(got, ref)
    seen[0] = max(seen[0], w)
    assert w <= 1.0, (section, what, w)


def _report(section, seen):
    print(f"\n[edge-bars] {section}: largest error / bar = {seen[0]:.3f}")


# ---- 2. deformation tail ------------------------------------------------------------------------------------
def _tail(base, deltas, ups, use):
    """deform_tail + autograd from the outputs selected by `use`: (outputs, base gradients, delta gradients)."""
    from gs4d_train.kernels import deform_tail
    b = [t.clone().requires_grad_(True) for t in base]
    d = [None if t is None else t.clone().requires_grad_(True) for t in deltas]
    out = deform_tail(*b, *d)
    loss = sum((o * u).sum() for o, u, k in zip(out, ups, use) if k)
    grads = torch.autograd.grad(loss, b + [t for t in d if t is not None], allow_unused=True)
    rest = iter(grads[6:])
    return out, grads[:6], [None if t is None else next(rest) for t in d]


@pytest.mark.parametrize("heads", ["all", "none", "mixed"])
@pytest.mark.parametrize("P,K", [(257, 1), (257, 4), (257, 9), (257, 16), (1, 1), (1, 16)])
def test_deform_tail_edges(P, K, heads):
    """kernels.deform_tail at every SH width (3K % 4 == 0: the float4 form, K = 4, 16; the scalar form, K = 1 with
    f_rest = NULL, K = 9), one row past a 256-thread group and a single row, with all / no / some heads, on rows
    planted at r + dr == 0, |r + dr| = 3e-13 (below eps), components 1e-25 (squares underflow), 2e-12 (just above
    eps), 1e15, s + ds in {-80, 0, 80} and o + do in {-100, -20, 0, 20, 100}: outputs and every gradient within the
    fp64 bars, finite on the planted rows, the heads' gradients bitwise the bases'; then with only (means, shs) and
    only opac used downstream: the unused branches' gradients are exact zeros (d_dshs included).
    The zero-norm rows gave NaN rotation gradients (0 * (0 / 0), 0 * inf) before the backward stopped dividing by
    the unclamped norm at or below eps; F.normalize's graph gives g / 1e-12 there."""
    base, deltas, ups = R.deform_inputs(P, K, heads, DEV)
    rows = R.planted_rows(P)
    seen, seen_add = [0.0], [0.0]  # (a single add's bar is its worst case: reached by construction)
    for use in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 1), (0, 0, 0, 1, 0)):
        out, gb, gd = _tail(base, deltas, ups, use)
        ro, rg = R.deform_tail_ref(base, deltas, [u if k else None for u, k in zip(ups, use)])
        if all(use):
            for o, k in zip(out, ("means", "scales", "rot", "opac", "shs")):
                _hold("deform_tail", o, ro[k], (k, use), seen_add if k in ("means", "shs") else seen)
        for g, k in zip(gb, ("d_xyz", "d_s", "d_r", "d_o", "d_fdc", "d_frest")):
            assert g is not None and bool(torch.isfinite(g[rows]).all()), (k, use, g[rows])
            _hold("deform_tail", g, rg[k], (k, use), seen)
        for i in range(4):  # the heads' gradients: the same values in buffers of their own
            assert (gd[i] is None) == (deltas[i] is None)
            if gd[i] is not None:
                assert gd[i].data_ptr() != gb[i].data_ptr() and torch.equal(gd[i], gb[i]), (i, use)
        if deltas[4] is not None:
            assert gd[4].shape == (P, 3 * K)
            _hold("deform_tail", gd[4], rg["d_shs"], ("d_dshs", use), seen)
            assert torch.equal(gd[4], torch.cat((gb[4], gb[5]), dim=1).reshape(P, 3 * K))
    _report(f"2 deform_tail P={P} K={K} {heads}", seen)
    _report(f"2 deform_tail P={P} K={K} {heads} (means, shs: one add)", seen_add)


@pytest.mark.parametrize("K", [1, 16])
def test_deform_tail_no_rows(K):
    """P = 0: empty outputs of the right shapes, and the backward returns empty gradients."""
    base, deltas, ups = R.deform_inputs(0, K, "all", DEV)
    out, gb, gd = _tail(base, deltas, ups, (1, 1, 1, 1, 1))
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, K, 3)]
    assert [tuple(g.shape) for g in gb] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, 1, 3), (0, K - 1, 3)]
    assert [tuple(g.shape) for g in gd] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, 3 * K)]


# ---- 3. densification statistics ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["visible+radii", "radii", "visible"])
@pytest.mark.parametrize("P", [0, 1, 257])
def test_densify_stats_edges(P, form):
    """kernels.densify_stats in the three mask forms -- (visible, radii), (None, radii): radii > 0 inside the
    kernel, the fused step's form, (visible, None): max_radii2D untouched -- with radii that contain zeros, rows
    visible with radius 0, (P, 1) accumulators and a non-contiguous viewspace gradient: denom and max_radii2D
    exact, rows outside the mask bitwise untouched, grad_accum within sqrt + two products + two adds."""
    from gs4d_train.kernels import densify_stats
    vs4, vis, radii, acc, den, mr = R.densify_inputs(P, DEV)
    v = vis if "visible" in form else None
    r = radii if "radii" in form else None
    vs = vs4[:, :3]
    assert P < 2 or not vs.is_contiguous()
    ref, rden, rmr, mask = R.densify_stats_ref(vs, v, r, acc, den, mr)
    if P > 1:
        assert bool((mask & (radii == 0)).any()) == (v is not None) and bool((~mask).any())
    acc0, den0, mr0 = acc.clone(), den.clone(), mr.clone()
    densify_stats(vs, v, r, acc, den, mr)
    seen = [0.0]
    _hold("densify_stats", acc, ref, "grad_accum", seen)
    assert torch.equal(den.double(), rden) and torch.equal(mr.double(), rmr)
    assert torch.equal(acc[~mask], acc0[~mask]) and torch.equal(den[~mask], den0[~mask])
    assert torch.equal(mr[~mask], mr0[~mask])
    if r is None:
        assert torch.equal(mr, mr0)
    if P:
        assert bool((den[mask] == den0[mask] + 1).all())
    _report(f"3 densify_stats P={P} {form}", seen)


# ---- 4. FusedAdam ---------------------------------------------------------------------------------------------
def _adam_groups(params, two_groups):
    if not two_groups:
        return [{"params": params, "betas": R.ADAM_HYPER[0][0], "eps": R.ADAM_HYPER[0][1]}]
    return [{"params": params[:60], "betas": R.ADAM_HYPER[0][0], "eps": R.ADAM_HYPER[0][1]},
            {"params": params[60:], "betas": R.ADAM_HYPER[1][0], "eps": R.ADAM_HYPER[1][1]}]


def _state(opt, p):
    st = opt.state[p]
    if not st:
        return torch.zeros_like(p), torch.zeros_like(p), 0.0
    return st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])


@pytest.mark.parametrize("n,two_groups", [(48, False), (49, False), (50, False), (97, False), (97, True)])
def test_fused_adam_edges(n, two_groups):
    """FusedAdam with as many tensors as one launch takes (48, GS4D_ADAM_MAX_TENSORS), one and two more (the
    second launch's chunk numbering restarts; at 49 it holds the zero-element last parameter alone, at 50 a real
    one too) and 97 (three launches), in one param group and in two with different betas and eps (60 + 37: the
    first still needs two launches).  Sizes cycle through 1, 3, 4, 5, 130, 4095, 4096 (one chunk), 4097, 4099
    (a float4 tail in a second chunk) and 8194; every other parameter is stored 4 bytes off 16-byte alignment (the
    scalar path); two have zero elements; one gradient is a transposed view; one is None at the second step (its
    tensor, moments and step count stay as they are).  Gradients hold an exact 0 (the parameter stays bitwise
    unchanged), 1e-25 (g * g underflows), +-1e18 and randn * {1e-3, 1, 1e3}.  Each of three steps is checked
    against the fp64 formula started from the tensors before that step; step counts equal torch.optim.Adam's; an
    optimizer of more than 48 parameters gives bitwise the result of two optimizers of 48 and the rest."""
    from gs4d_train.kernels import FusedAdam
    params = [torch.nn.Parameter(p) for p in R.adam_case(n, DEV)]
    assert sum(p.data_ptr() % 16 == 4 for p in params) >= n // 2 - 2
    first = [p.detach().clone() for p in params]
    opt = FusedAdam(_adam_groups(params, two_groups), lr=R.ADAM_LR)
    twin_p = [torch.nn.Parameter(p.detach().clone()) for p in params]
    twin = torch.optim.Adam(_adam_groups(twin_p, two_groups), lr=R.ADAM_LR)
    split_p = [torch.nn.Parameter(p) for p in R.adam_case(n, DEV)]
    split = [FusedAdam(_adam_groups(split_p[:48], False), lr=R.ADAM_LR)]
    if n > 48:
        split.append(FusedAdam(_adam_groups(split_p[48:], False), lr=R.ADAM_LR))
    seen = [0.0]
    for step in range(3):
        grads = R.adam_grads(params, step)
        before = [(p.detach().clone(),) + _state(opt, p) for p in params]
        for ps in (params, twin_p, split_p):
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.clone() if g.is_contiguous() else g
        assert not grads[4].is_contiguous() and (grads[5] is None) == (step == 1)
        opt.step()
        twin.step()
        for o in split:
            o.step()
        for i, (p, g, (p0, m0, v0, t0)) in enumerate(zip(params, grads, before)):
            m1, v1, t1 = _state(opt, p)
            if g is None:
                assert torch.equal(p, p0) and torch.equal(m1, m0) and torch.equal(v1, v0) and t1 == t0 == 1.0
                continue
            (b1, b2), eps = R.ADAM_HYPER[1 if two_groups and i >= 60 else 0]
            rm, rv, rp = R.adam_ref(p0, g, m0, v0, b1, b2, eps, *R.adam_scalars(R.ADAM_LR, b1, b2, t0 + 1))
            _hold("adam", m1, rm, (step, i, "exp_avg"), seen)
            _hold("adam", v1, rv, (step, i, "exp_avg_sq"), seen)
            _hold("adam", p, rp, (step, i, "param"), seen)
            assert t1 == t0 + 1
    for i, (p, q, f) in enumerate(zip(params, twin_p, first)):
        assert _state(opt, p)[2] == _state(twin, q)[2] == (2.0 if i == 5 else 3.0)
        if p.numel() >= 3:  # gradient exactly 0 at every step, zero moments: bitwise unchanged
            assert torch.equal(p.detach().reshape(-1)[0], f.reshape(-1)[0])
            assert float(opt.state[p]["exp_avg"].reshape(-1)[0]) == 0.0
    if not two_groups:
        for i, (p, q) in enumerate(zip(params, split_p)):
            so = split[0] if i < 48 else split[1]
            assert torch.equal(p, q), i
            assert torch.equal(opt.state[p]["exp_avg"], so.state[q]["exp_avg"]), i
            assert torch.equal(opt.state[p]["exp_avg_sq"], so.state[q]["exp_avg_sq"]), i
    _report(f"4 adam n={n} groups={1 + two_groups}", seen)


# ---- 5. L1 loss -----------------------------------------------------------------------------------------------
def test_l1_loss_edges():
    """The L1 kernels on one stream, large, small, large through the kept scratch: 33, 18, 16 and 17 workgroups (the
    last-workgroup total's 16 sub-counters: more than, exactly and one past the fan-in), 1 and 2 workgroups, n in
    1..5 and 8, n % 4 != 0 (the scalar kernels and l1_loss_and_grad's two-pass fallback) and == 0 (float4 / char4
    and the one-pass form), with exact ties, x - y = +1e-40 and -1e-40 (denormals: signs +1 and -1) in each tensor.
    The value within (8 + 3) * 2^-24 of the fp64 mean; the gradient exactly sign * fl32(dloss * fl32(1 / n)),
    through l1_loss + autograd and through l1_loss_and_grad, which agree bitwise."""
    from gs4d_train.kernels import l1_loss, l1_loss_and_grad
    seen = [0.0]
    dloss = 0.37
    for n in R.L1_SIZES:
        x, y = R.l1_inputs(n, DEV)
        ref, grad = R.l1_ref(x, y, dloss)
        xa = x.clone().requires_grad_(True)
        loss = l1_loss(xa, y)
        loss.backward(torch.tensor(dloss, device=DEV))
        loss2, grad2 = l1_loss_and_grad(x, y, dloss)
        _hold("l1", loss.detach(), ref, n, seen)
        assert torch.equal(xa.grad, grad), n
        assert torch.equal(loss2, loss.detach()) and torch.equal(grad2, grad), n
        if n >= 8:
            assert float(grad[0]) == 0.0 and float(grad[5]) == 0.0
        if n >= 3:
            assert float(grad[n - 1]) > 0.0 > float(grad[n - 2])
    _report("5 l1", seen)


@pytest.mark.parametrize("H", [37, 36])  # 3 * H * 29 % 4 != 0: the fallback; == 0: the one-pass form
def test_l1_loss_non_contiguous(H):
    """A permuted image (non-contiguous x) gives the loss and the gradient values of its contiguous clone."""
    from gs4d_train.kernels import l1_loss, l1_loss_and_grad
    g = torch.Generator().manual_seed(5)
    x = torch.rand(H, 29, 3, generator=g).to(DEV).permute(2, 0, 1)
    y = torch.rand(3, H, 29, generator=g).to(DEV)
    assert not x.is_contiguous()
    outs = []
    for t in (x, x.contiguous()):
        ta = t.detach().requires_grad_(True)
        loss = l1_loss(ta, y)
        loss.backward()
        loss2, grad2 = l1_loss_and_grad(t, y)
        assert torch.equal(loss2, loss.detach()) and torch.equal(grad2, ta.grad)
        outs.append((loss.detach(), ta.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref, grad = R.l1_ref(x, y, 1.0)
    assert R.worst(outs[0][0], ref) <= 1.0 and torch.equal(outs[0][1], grad)


# ---- 6. HexPlane field ----------------------------------------------------------------------------------------
def _small_field(F, multires):
    from gs4d_train.deformation import HexPlaneField
    torch.manual_seed(3)
    f = HexPlaneField(1.6, {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": F,
                            "resolution": [8, 6, 5, 3]}, list(multires)).to(DEV)
    with torch.no_grad():
        for level in f.grids:  # random time planes too (init is all-ones)
            for p in level:
                p.uniform_(0.1, 1.2)
    return f


def _hex_points(N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(N, 4, generator=g) * 2.4 - 1.2  # incl. border-clamped coordinates
    if kind == "same":
        pts = pts[:1].clamp(-0.9, 0.9).repeat(N, 1)
    elif N >= 63:  # rows exactly on the borders
        pts[0:8, 0] = 1.0
        pts[8:16, 3] = -1.0
        pts[16:20, 1] = -1.0
        pts[20:24, 2] = 1.0
        pts[24] = 1.0
        pts[25] = -1.0
    return pts.to(DEV)


@pytest.mark.parametrize("F", [4, 32])
@pytest.mark.parametrize("multires", [(1,), (1, 2, 4), (1, 2, 4, 8)])
def test_hexplane_small_distinct_planes(multires, F):
    """The fused field with resolution (8, 6, 5, 3): all four sizes distinct, so every plane has W != H and a swapped
    W / H or coordinate pair shows; 1, 3 and 4 levels (GS4D_HEXPLANE_MAX_LEVELS: the backward's per-level histogram
    and scale words), F = 4 and 32, N in {0, 1, 63, 257, 3000} points in [-1.2, 1.2] with rows exactly at +-1, and 257
    identical points (every tap in one cell).  Against interpolate_ms_features on float64 copies of the planes and
    points: features to rtol 1e-5 / atol 1e-6, the point gradients and every plane gradient to 1e-4 of the tensor's
    max; two backward passes bitwise equal; N = 0: empty features, all-zero plane gradients."""
    from gs4d_train.deformation import interpolate_ms_features
    from gs4d_train.kernels import hexplane
    f = _small_field(F, multires)
    L = len(multires)
    sizes = [tuple(p.shape[2:]) for p in f.grids[0]]
    assert sizes == [(6, 8), (5, 8), (3, 8), (5, 6), (3, 6), (3, 5)]  # (H, W) = (reso[c1], reso[c0])
    planes = [p for level in f.grids for p in level]
    grids = [list(level) for level in f.grids]
    grids64 = [[p.detach().double().requires_grad_(True) for p in level] for level in f.grids]
    planes64 = [p for level in grids64 for p in level]
    seen_f, seen_b = [0.0], [0.0]
    for N, kind in ((0, "rand"), (1, "rand"), (63, "rand"), (257, "rand"), (257, "same"), (3000, "rand")):
        pts = _hex_points(N, kind, 100 + N).requires_grad_(True)
        feat = hexplane(pts, grids)
        assert feat.shape == (N, L * F)
        up = torch.randn(N, L * F, generator=torch.Generator().manual_seed(N)).to(DEV)
        got = torch.autograd.grad(feat, [pts] + planes, up, retain_graph=True)
        again = torch.autograd.grad(feat, [pts] + planes, up)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        if N == 0:
            assert got[0].shape == (0, 4) and all(not bool(g.any()) and g.shape == p.shape
                                                  for g, p in zip(got[1:], planes))
            continue
        p64 = pts.detach().double().requires_grad_(True)
        ref = interpolate_ms_features(p64, grids64).reshape(N, L * F)
        want = torch.autograd.grad(ref, [p64] + planes64, up.double())
        err = (feat.detach().double() - ref.detach()).abs()
        seen_f[0] = max(seen_f[0], float((err / (1e-6 + 1e-5 * ref.detach().abs())).max()))
        torch.testing.assert_close(feat.detach(), ref.detach().float(), rtol=1e-5, atol=1e-6)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and bool(torch.isfinite(a).all())
            bar = 1e-4 * max(float(b.abs().max()), 1e-30)
            e = float((a.double() - b).abs().max())
            seen_b[0] = max(seen_b[0], e / bar)
            assert e <= bar, (N, kind, "pts" if k == 0 else f"plane {k - 1}", e, bar)
    _report(f"6 hexplane forward levels={L} F={F}", seen_f)
    _report(f"6 hexplane backward levels={L} F={F}", seen_b)
