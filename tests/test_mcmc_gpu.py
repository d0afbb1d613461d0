"""MCMC densification on the GPU (csrc/mcmc.hip, gs4d_train/mcmc.py) against tests/mcmc_refs.py.

Integers are compared bit for bit (the generator's words, the sampler's draws and counts).  A float tensor T is held
to e = max|T - T64| / max|T64| <= max(4 e_u, 1e-6), T64 the fp64 reference and e_u the error of the unfused fp32
formulation (gs4d_train.mcmc's torch / numpy functions) measured in the same test on the same inputs: the bar of
tests/test_rigidity_gpu.py and the deformation-route tests.  Every figure is printed before it is asserted."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcmc_refs as MR
import stream_cases as SC
import mcmc_models as TB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 63, 64, 65, 257, 1025, 4097)
MIN_O = 0.005


def _C():
    from gs4d_train import _C
    return _C


def rel_err(t, t64):
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    return float(np.abs(t - t64).max() / max(np.abs(t64).max(), 1e-300)) if t64.size else 0.0


def within(tag, figures):
    """figures: (name, e_f, e_u); prints them all, then asserts e_f <= max(4 e_u, 1e-6) for each"""
    print(f"[mcmc] {tag}: " + ", ".join(f"{n} e_f {ef:.2e} e_u {eu:.2e}" for n, ef, eu in figures), flush=True)
    for n, ef, eu in figures:
        assert ef <= max(4 * eu, 1e-6), (tag, n, ef, eu)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


# ---- the generator ----------------------------------------------------------------------------------------------------
def gpu_bits(n, seed, iteration, purpose):
    out = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)
    return _C().mcmc_random_bits(out, seed, iteration, purpose)


@pytest.mark.parametrize("n", SIZES)
def test_random_bits(n):
    for seed, it, purpose in ((0, 1, 0), ((5 << 32) + 7, 9, 2), (2 ** 64 - 1, 2 ** 32 - 1, 1)):
        want = torch.from_numpy(MR.blocks(n, seed, it, purpose).view(np.int32))
        assert torch.equal(gpu_bits(n, seed, it, purpose).cpu(), want), (n, seed, it, purpose)


def test_random_bits_refuses_bad_input():
    f = _C().mcmc_random_bits
    for bad in (lambda: f(torch.zeros(4, 4, dtype=torch.int32), 0, 0, 0),
                lambda: f(torch.zeros(4, 3, dtype=torch.int32, device=DEV), 0, 0, 0),
                lambda: f(torch.zeros(4, 4, device=DEV), 0, 0, 0),
                lambda: f(torch.zeros(4, 4, dtype=torch.int32, device=DEV), 0, -1, 0)):
        with pytest.raises(RuntimeError):
            bad()


# ---- the sampler ------------------------------------------------------------------------------------------------------
def opacities(P, seed=0):
    rng = np.random.default_rng(seed + P)
    o = rng.random(P).astype(np.float32)
    o[::3] = np.float32(0.001)  # a third dead
    return o


def gpu_sample(o, n, seed, it, purpose, min_opacity=MIN_O):
    draws, counts, drawn = _C().mcmc_sample(dev(o), min_opacity, n, seed, it, purpose)
    return draws.cpu().numpy(), counts.cpu().numpy(), int(drawn.item())


def assert_sample(o, n, seed=(3 << 32) + 1, it=700, purpose=MR.RELOCATE):
    got, want = gpu_sample(o, n, seed, it, purpose), MR.sample(o, MIN_O, n, seed, it, purpose)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (len(o), n)
    again = gpu_sample(o, n, seed, it, purpose)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    return got


@pytest.mark.parametrize("P", SIZES)
def test_sample_matches_the_reference(P):
    o = opacities(P)
    for n in (0, 1, P // 4, 3 * P):
        assert_sample(o, n)
    if P >= 63:
        assert_sample(o, P // 4, purpose=MR.GROW)
        a, b = gpu_sample(o, P // 4, 1, 700, 1)[0], gpu_sample(o, P // 4, 1, 701, 1)[0]
        assert not np.array_equal(a, b)  # another iteration, other draws


LARGE = (65537, 131100)  # 257 and 513 tiles of 256 rows: the tile-sum scan's second and third chunk of 256 tiles


@pytest.mark.parametrize("P", LARGE)
def test_sample_crosses_the_tile_scan_chunks(P):
    """mcmc_tile_scan_kernel scans the tile sums 256 at a time with a carry: above 65,536 rows the loop runs more than
    once (every training run's case).  A third of the rows dead, the rest live in every chunk; then two live rows only,
    one in the first tile and one in the last chunk, where a lost carry moves every draw of the last row"""
    o = opacities(P)
    d, c, drawn = assert_sample(o, 2000)
    assert drawn == 2000 and int(d.max()) >= P - 1024 and int(d.min()) < 1024 and int(c.sum()) == 2000
    two = np.full(P, 0.001, np.float32)
    two[3], two[P - 1] = 0.25, 0.75  # row P - 1 lies in the last chunk's last tile at both sizes
    d, c, drawn = assert_sample(two, 400, purpose=MR.GROW)
    print(f"[mcmc] sampler P={P}: rows 3 and {P - 1} (0.25 : 0.75) took {c[3]} and {c[P - 1]} of 400 draws", flush=True)
    assert drawn == 400 and c[3] + c[P - 1] == 400 and 60 <= c[3] <= 140


def test_sample_special_cases():
    P = 257
    one = np.full(P, 0.004, np.float32)
    one[200] = 0.3
    d, c, drawn = assert_sample(one, 3 * P)
    assert drawn == 3 * P and (d == 200).all() and c[200] == 3 * P and c.sum() == 3 * P
    d, c, drawn = assert_sample(np.full(P, 0.005, np.float32), 50)  # opacity == min_opacity is dead
    assert drawn == 0 and not d.any() and not c.any()
    d, c, drawn = assert_sample(np.full(P, 0.25, np.float32), 3 * P)
    assert drawn == 3 * P and c.min() >= 0 and c.max() <= 12 and len(np.unique(d)) > P // 2
    heavy = np.full(P, 0.006, np.float32)
    heavy[77] = np.float32(1 - 2.0 ** -24)
    d, c, drawn = assert_sample(heavy, 3 * P)
    print(f"[mcmc] sampler: the row of opacity 1 - 2^-24 among 256 of 0.006 took {c[77]} of {3 * P} draws", flush=True)
    assert 0.25 < c[77] / (3 * P) < 0.55  # 1 / (1 + 256 * 0.006) = 0.39 of the weight


def test_sample_refuses_bad_input():
    f = _C().mcmc_sample
    for bad in (lambda: f(torch.rand(8), MIN_O, 4, 0, 0, 1), lambda: f(torch.rand(8, 2, device=DEV), MIN_O, 4, 0, 0, 1),
                lambda: f(torch.rand(8, device=DEV), -1.0, 4, 0, 0, 1), lambda: f(torch.rand(8, device=DEV), MIN_O, -4, 0, 0, 1),
                lambda: f(torch.rand(8, device=DEV).double(), MIN_O, 4, 0, 0, 1)):
        with pytest.raises(RuntimeError):
            bad()


# ---- the correction ---------------------------------------------------------------------------------------------------
def relocate_inputs(P, seed=0):
    rng = np.random.default_rng(seed + 7)
    o = rng.uniform(0.0051, 0.999, P)
    counts = rng.integers(0, 4, P).astype(np.int32)
    k = min(P, 8)
    o[:k] = (0.0050001, 0.0050001, 0.3, 0.9, 0.999, 0.999, 0.02, 0.5)[:k]
    counts[:k] = (60, 1, 50, 51, 49, 2, 60, 0)[:k]  # beyond the clamp at n = 51, and an untouched row
    raw_o = np.log(o / (1 - o)).astype(np.float32).reshape(P, 1)
    raw_s = rng.normal(-3, 1, (P, 3)).astype(np.float32)
    return raw_o, raw_s, counts


@pytest.mark.parametrize("P", SIZES)
def test_relocate_matches_fp64_within_the_unfused_bar(P):
    """measured on an MI355X in DESIGN 10.16"""
    from gs4d_train import mcmc
    raw_o, raw_s, counts = relocate_inputs(P)
    o, s, c = dev(raw_o), dev(raw_s), dev(counts, torch.int32)
    _C().mcmc_relocate(o, s, c, MIN_O)
    if P == 0:
        return
    got_o, got_s = o.cpu().numpy(), s.cpu().numpy()
    untouched = counts == 0
    assert np.array_equal(got_o[untouched].view(np.int32), raw_o[untouched].view(np.int32))
    assert np.array_equal(got_s[untouched].view(np.int32), raw_s[untouched].view(np.int32))
    touched = ~untouched
    if not touched.any():
        return
    want_o, want_s = MR.relocate_rows(raw_o, raw_s, counts, MIN_O)
    rows, u_o, u_s = mcmc.corrected_torch(dev(raw_o), dev(raw_s), c, MIN_O)
    assert np.array_equal(rows.cpu().numpy(), np.nonzero(touched)[0])
    within(f"relocate P={P}", [("opacity", rel_err(got_o[touched], want_o[touched]), rel_err(u_o.cpu().numpy(), want_o[touched])),
                               ("scaling", rel_err(got_s[touched], want_s[touched]), rel_err(u_s.cpu().numpy(), want_s[touched]))])
    assert np.isfinite(got_o).all() and np.isfinite(got_s).all()


# ---- the noise --------------------------------------------------------------------------------------------------------
def noise_inputs(P, seed=0):
    rng = np.random.default_rng(seed + 11)
    raw_o = rng.normal(-1, 2, (P, 1)).astype(np.float32)
    raw_o[4::5] = np.float32(np.log(0.999 / 0.001))  # opacity 0.999: the gate closes (row 0 stays open: P = 1 moves)
    return dict(xyz=rng.normal(size=(P, 3)).astype(np.float32), s=rng.normal(-3, 0.7, (P, 3)).astype(np.float32),
                r=rng.normal(size=(P, 4)).astype(np.float32), o=raw_o, z=rng.normal(size=(P, 3)).astype(np.float32))


@pytest.mark.parametrize("P", SIZES)
def test_noise_with_given_normals(P):
    from gs4d_train import mcmc
    t = noise_inputs(P)
    step = 37.5
    zero = torch.zeros(P, 3, device=DEV)  # from zero, the stored position IS the change
    s, r, o, z = dev(t["s"]), dev(t["r"]), dev(t["o"]), dev(t["z"])
    _C().mcmc_noise(zero, s, r, o, step, 0, 0, z)
    if P == 0:
        return
    got = zero.cpu().numpy()
    want = MR.noise_delta(t["s"], t["r"], t["o"], step, t["z"])
    unfused = mcmc.noise_delta_torch(s, r, o, step, z).cpu().numpy()
    within(f"noise (given normals) P={P}", [("dx", rel_err(got, want), rel_err(unfused, want))])
    gated = np.arange(P) % 5 == 4
    scale = np.exp(t["s"].astype(np.float64)).max(1)
    assert P < 5 or (np.abs(got[gated]).max(1) < 1e-30 * scale[gated]).all()
    assert np.abs(got[~gated]).max() > 0
    # in place on real positions: x + dx, rounded once
    x = dev(t["xyz"])
    _C().mcmc_noise(x, s, r, o, step, 0, 0, z)
    assert torch.equal(x, dev(t["xyz"]) + zero)


@pytest.mark.parametrize("P", SIZES)
def test_noise_with_generated_normals(P):
    """unit scales, the identity rotation and an open gate: the change is z g step_scale, so the kernel's normals are
    read back from it and held against fp64 Box-Muller of the exact words, numpy-fp32 Box-Muller giving e_u"""
    seed, it, step = (9 << 32) + 4, 3100, 0.5
    s, o = torch.zeros(P, 3, device=DEV), torch.full((P, 1), -20.0, device=DEV)
    r = torch.zeros(P, 4, device=DEV)
    r[:, 0] = 1
    x = torch.zeros(P, 3, device=DEV)
    _C().mcmc_noise(x, s, r, o, step, seed, it, None)
    again = torch.zeros(P, 3, device=DEV)
    _C().mcmc_noise(again, s, r, o, step, seed, it, None)
    assert torch.equal(x, again)  # bitwise repeatable
    if P == 0:
        return
    other = torch.zeros(P, 3, device=DEV)
    _C().mcmc_noise(other, s, r, o, step, seed, it + 1, None)
    assert not torch.equal(x, other)  # another iteration, other bits
    words = MR.blocks(P, seed, it, MR.NOISE)
    assert torch.equal(gpu_bits(P, seed, it, MR.NOISE).cpu(), torch.from_numpy(words.view(np.int32)))
    sn, rn, on = np.zeros((P, 3)), np.tile([1.0, 0, 0, 0], (P, 1)), np.full((P, 1), -20.0)
    z = MR.implied_normals(x.cpu().numpy(), sn, rn, on, step)
    z64, z32 = MR.normals64(words), MR.normals32(words)
    print(f"[mcmc] generated normals P={P}: kernel {np.abs(z - z64).max():.2e} absolute, numpy fp32 "
          f"{np.abs(z32 - z64).max():.2e}", flush=True)
    within(f"noise (generated normals) P={P}", [("z", rel_err(z, z64), rel_err(z32, z64))])


def test_noise_refuses_bad_input():
    f = _C().mcmc_noise
    P = 8
    x, s, r, o = (torch.zeros(P, k, device=DEV) for k in (3, 3, 4, 1))
    for bad in (lambda: f(x.cpu(), s, r, o, 1.0, 0, 0, None), lambda: f(x, s[:4], r, o, 1.0, 0, 0, None),
                lambda: f(x, s, r[:, :3], o, 1.0, 0, 0, None), lambda: f(x, s, r, o, 1.0, 0, 0, x.cpu()),
                lambda: f(x, s, r, o, 1.0, 0, 2 ** 32, None)):
        with pytest.raises(RuntimeError):
            bad()


# ---- the regulariser --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_reg_grad(P):
    t = noise_inputs(P, seed=3)
    o, s = dev(t["o"]), dev(t["s"])
    base_o, base_s = dev(t["z"][:, :1].copy()), dev(t["xyz"])  # non-zero buffers: the gradient is ADDED
    go, gs = base_o.clone(), base_s.clone()
    wo, ws = 0.01, 0.02
    value = _C().mcmc_reg_grad(o, s, wo, ws, go, gs)
    go2, gs2 = base_o.clone(), base_s.clone()
    value2 = _C().mcmc_reg_grad(o, s, wo, ws, go2, gs2)
    assert SC.first_difference([value, go, gs], [value2, go2, gs2]) is None  # two calls, the same bits
    only_value = _C().mcmc_reg_grad(o, s, wo, ws, None, None)
    assert SC.first_difference([only_value], [value]) is None
    if P == 0:
        assert float(value) == 0.0
        return
    v64, go64, gs64 = MR.regulariser(t["o"], t["s"], wo, ws)
    sig, ex = torch.sigmoid(o), torch.exp(s)
    v_u = wo * sig.mean() + ws * ex.mean()
    go_u, gs_u = (wo / P) * (sig * (1 - sig)), (ws / (3 * P)) * ex
    # the gradient itself from zero buffers (0 + g is g: nothing cancels), then ADDED to what a buffer holds: base + g,
    # rounded once
    zo, zs = torch.zeros_like(base_o), torch.zeros_like(base_s)
    value0 = _C().mcmc_reg_grad(o, s, wo, ws, zo, zs)
    assert SC.first_difference([value0, go, gs], [value, base_o + zo, base_s + zs]) is None
    assert bool((go != base_o).any()) and bool((gs != base_s).any())
    within(f"reg_grad P={P}", [("value", rel_err(value.cpu().numpy(), v64), rel_err(v_u.cpu().numpy(), v64)),
                               ("d opacity", rel_err(zo.cpu().numpy(), go64), rel_err(go_u.cpu().numpy(), go64)),
                               ("d scaling", rel_err(zs.cpu().numpy(), gs64), rel_err(gs_u.cpu().numpy(), gs64))])


# ---- moment zeroing ---------------------------------------------------------------------------------------------------
def test_zero_rows():
    P = 1025
    g = torch.Generator().manual_seed(5)
    shapes = [(P, 3), (P, 3), (P, 1, 3), (P, 1, 3), (P, 15, 3), (P, 15, 3), (P, 1), (P, 1), (P, 3), (P, 3), (P, 4), (P, 4)]
    tensors = [(torch.randn(sh, generator=g) + 3.0).to(DEV) for sh in shapes]
    before = [t.clone() for t in tensors]
    rows = torch.randint(0, P, (300,), generator=g).to(torch.int32)
    rows[10:20] = rows[0:10]  # duplicates
    rows[-1] = P - 1
    _C().mcmc_zero_rows(tensors, rows.to(DEV))
    listed = torch.zeros(P, dtype=torch.bool)
    listed[rows.long()] = True
    for t, b in zip(tensors, before):
        t, b = t.cpu(), b.cpu()
        assert not t[listed].any() and SC.first_difference([t[~listed]], [b[~listed]]) is None
    _C().mcmc_zero_rows(tensors, rows[:0].to(DEV))  # an empty list
    _C().mcmc_zero_rows([], rows.to(DEV))
    with pytest.raises(RuntimeError):
        _C().mcmc_zero_rows(tensors, rows)  # a CPU row list
    with pytest.raises(RuntimeError):
        _C().mcmc_zero_rows(tensors + [torch.zeros(P - 1, 3, device=DEV)], rows.to(DEV))


# ---- relocate / grow: the fused model against the CPU formulation ---------------------------------------------------------
def model_pair(P, dead):
    """a CPU model with non-zero moments and statistics (tests/test_mcmc_boundary.py's) and its fused copy on the GPU"""
    from gs4d_train.gaussians import GaussianModel
    gc, hyper, opt = TB.make_model(P=P, seed=3, dead=dead)
    gg = GaussianModel(3, hyper, fused=True)
    for a in TB.PARAM_ATTRS:
        setattr(gg, a, torch.nn.Parameter(getattr(gc, a).detach().to(DEV)))
    gg.max_radii2D, gg._deformation_table, gg.spatial_lr_scale = gc.max_radii2D.to(DEV), gc._deformation_table.to(DEV), 1.0
    gg._deformation = gg._deformation.to(DEV)
    gg.training_setup(opt)
    gg.optimizer.load_state_dict(gc.optimizer.state_dict())
    for name in ("xyz_gradient_accum", "denom", "_deformation_accum"):
        setattr(gg, name, getattr(gc, name).to(DEV))
    return gc, gg


def assert_models_agree(tag, gc, gg, gc64):
    """the same rows in the same order: parameters within the relocate bar (e_u: the CPU formulation against the fp64
    rows), integer and bool tensors equal, moments equal"""
    sc, sg = TB.snapshot(gc), TB.snapshot(gg)
    figures = []
    for a in TB.PARAM_ATTRS:
        assert sc[a].shape == sg[a].shape, a
        if a in gc64:
            figures.append((a, rel_err(sg[a].cpu().numpy(), gc64[a]), rel_err(sc[a].numpy(), gc64[a])))
        else:  # copies
            assert SC.first_difference([sg[a].cpu()], [sc[a]]) is None, a
    within(tag, figures)
    assert torch.equal(sg["table"].cpu(), sc["table"])
    assert len(sg["moments"]) == len(sc["moments"]) == 12
    for x, y in zip(sg["moments"] + sg["stats"], sc["moments"] + sc["stats"]):
        assert SC.first_difference([x.cpu()], [y]) is None


def test_relocate_and_grow_fused_against_cpu():
    from gs4d_train import mcmc
    P = 1025
    dead = tuple(range(5, P, 9))
    gc, gg = model_pair(P, dead)
    raw_o, raw_s = gc._opacity.detach().numpy().copy(), gc._scaling.detach().numpy().copy()
    opacity = gc.get_opacity.detach().reshape(-1).numpy()
    assert torch.equal(gg.get_opacity.detach().cpu() <= MIN_O, gc.get_opacity.detach() <= MIN_O)
    draws, counts, _ = MR.sample(opacity, MIN_O, len(dead), 11, 700, MR.RELOCATE)
    o64, s64 = MR.relocate_rows(raw_o, raw_s, counts, MIN_O)
    o64[list(dead)], s64[list(dead)] = o64[draws], s64[draws]
    assert mcmc.relocate(gc, 11, 700, MIN_O) == mcmc.relocate(gg, 11, 700, MIN_O) == len(dead)
    assert gg._xyz.is_cuda and gg.row_generation == gc.row_generation
    assert_models_agree("relocate, fused against CPU", gc, gg, {"_opacity": o64, "_scaling": s64})
    # growth from the CPU model's state on both sides (the GPU's rows differ from it in the last place)
    gc, gg = model_pair(P, dead=())
    raw_o, raw_s = gc._opacity.detach().numpy().copy(), gc._scaling.detach().numpy().copy()
    n_new = int(1.05 * P) - P
    draws, counts, _ = MR.sample(gc.get_opacity.detach().reshape(-1).numpy(), MIN_O, n_new, 11, 700, MR.GROW)
    o64, s64 = MR.relocate_rows(raw_o, raw_s, counts, MIN_O)
    o64, s64 = np.concatenate([o64, o64[draws]]), np.concatenate([s64, s64[draws]])
    assert mcmc.grow(gc, 11, 700, 10 ** 6, MIN_O) == mcmc.grow(gg, 11, 700, 10 ** 6, MIN_O) == n_new
    assert gg._xyz.shape[0] == int(1.05 * P)
    assert_models_agree("grow, fused against CPU", gc, gg, {"_opacity": o64, "_scaling": s64})
    assert mcmc.grow(gg, 11, 701, int(1.05 * P), MIN_O) == 0  # at the cap


# ---- one fused train step ---------------------------------------------------------------------------------------------
TRAIN_ITERATION = 3002
N_DEAD = 50


def train_model(strategy, noise_lr=None):
    """the suite's smallest synthetic scene (tests/test_streams_gpu.py's: 2000 points, two 96 x 64 views), the first
    N_DEAD rows dead; iteration 3002 is a refinement iteration"""
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    hyper, opt = config.dynerf()
    opt.densify_from_iter, opt.densification_interval = 0, 2
    opt.densify_strategy, opt.mcmc_seed = strategy, (6 << 32) + 5
    if noise_lr is not None:
        opt.mcmc_noise_lr = noise_lr
    pts, cols = make_point_cloud(2000, seed=5)
    views = make_training_views(2, 96, 64, seed=6)
    torch.manual_seed(7)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = True
    g._deformation.deformation_net.fused_heads = True
    g.training_setup(opt)
    g.active_sh_degree = 3
    with torch.no_grad():
        g._opacity[:N_DEAD] = -8.0
    return g, hyper, opt, views


def train_once(strategy, noise_lr=None):
    from gs4d_train.train import train_step
    g, hyper, opt, views = train_model(strategy, noise_lr)
    before = (g._opacity.detach().cpu().numpy().copy(), g._scaling.detach().cpu().numpy().copy())
    loss = train_step(g, views, opt, hyper, TRAIN_ITERATION, torch.ones(3, device=DEV))
    torch.cuda.synchronize()
    return g, opt, loss, before


def digest(g, loss):
    h = hashlib.sha256()
    for t in [loss] + [getattr(g, a) for a in TB.PARAM_ATTRS] + [g._deformation_table] + TB.moments(g):
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_train_step_with_mcmc():
    from gs4d_train import mcmc
    g, opt, loss, before = train_once("mcmc")
    P0, P1 = 2000, int(1.05 * 2000)
    assert g._xyz.shape[0] == P1 == min(opt.mcmc_cap_max, P1)
    o_min = float(g.get_opacity.detach().min())
    print(f"[mcmc] train step: P {P0} -> {g._xyz.shape[0]}, smallest opacity {o_min:.4f}, loss {float(loss):.6f}", flush=True)
    # This scene never reaches the correction's clamp (its smallest opacity is printed above).  A source clamped to
    # min_opacity is stored as logit(min_opacity), whose fp32 sigmoid may land one ulp below min_opacity; such a row is
    # dead again at the next refinement and is relocated then (as in gsplat), so on a scene that reaches the clamp
    # this assertion would have to allow that ulp.
    assert not bool((g.get_opacity.detach() < opt.mcmc_min_opacity).any())
    assert all(m.shape[0] == P1 for m in TB.moments(g)) and g._deformation_table.shape[0] == P1
    # the loss carries the regulariser: the default strategy's loss on the same model plus the reference's value
    _, _, loss_default, _ = train_once("default")
    reg = MR.regulariser(before[0], before[1], opt.mcmc_opacity_reg, opt.mcmc_scale_reg)[0]
    print(f"[mcmc] train step: loss {float(loss):.6f} = {float(loss_default):.6f} + {reg:.6f}", flush=True)
    assert reg > 0 and abs(float(loss) - (float(loss_default) + reg)) <= 1e-5 * abs(float(loss))
    # the noise: against a run with mcmc_noise_lr = 0, everything but _xyz is bit for bit the same and _xyz differs by
    # the reference's change (e_u: the torch formulation's change added to the same positions in fp32)
    quiet, _, loss_quiet, _ = train_once("mcmc", noise_lr=0.0)
    assert SC.first_difference([loss_quiet], [loss]) is None
    for a in TB.PARAM_ATTRS[1:]:
        assert SC.first_difference([getattr(quiet, a)], [getattr(g, a)]) is None, a
    xyz_lr = next(q["lr"] for q in g.optimizer.param_groups if q["name"] == "xyz")
    step = float(opt.mcmc_noise_lr) * float(xyz_lr)
    s, r, o = (getattr(quiet, a).detach() for a in ("_scaling", "_rotation", "_opacity"))
    words = MR.blocks(P1, opt.mcmc_seed, TRAIN_ITERATION, MR.NOISE)
    want = MR.noise_delta(s.cpu().numpy(), r.cpu().numpy(), o.cpu().numpy(), step, MR.normals64(words))
    x0 = quiet._xyz.detach()
    got = (g._xyz.detach().double() - x0.double()).cpu().numpy()
    z32 = torch.from_numpy(mcmc.normals_numpy(P1, opt.mcmc_seed, TRAIN_ITERATION)).to(DEV)
    x_u = x0 + mcmc.noise_delta_torch(s, r, o, step, z32)
    unfused = (x_u.double() - x0.double()).cpu().numpy()
    print(f"[mcmc] train step: step_scale {step:.3f}, largest move {np.abs(want).max():.3e}", flush=True)
    assert np.abs(want).max() > 0
    within("train step's noise", [("dx", rel_err(got, want), rel_err(unfused, want))])
    # another process takes the same step to the same bits (the draws are a function of (seed, iteration)).
    # tests/gpu_helpers.py holds the rasterizer / oracle call helpers and nothing that starts a process; the suite's
    # cross-process checks (test_train_gpu.py, test_ssim_gpu.py) each run a `python -c` child as this one does.  Here the
    # child imports this module, so both processes run the same train_once and digest.
    tests = os.path.dirname(os.path.abspath(__file__))
    child = ("import sys; sys.path[:0] = [%r, %r]; import test_mcmc_gpu as T; g, _, loss, _ = T.train_once('mcmc'); "
             "print(T.digest(g, loss))" % (tests, os.path.join(os.path.dirname(tests), "4dgaussians-fast-train_amd")))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=55)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == digest(g, loss)


# ---- side streams and a second device -----------------------------------------------------------------------------------
CASE_P = 4097


def _case_inputs(seed):
    t = noise_inputs(CASE_P, seed=seed)
    raw_o, raw_s, counts = relocate_inputs(CASE_P, seed=seed)
    rows = np.random.default_rng(seed).integers(0, CASE_P, 500).astype(np.int32)
    return SC._od(xyz=torch.tensor(t["xyz"]), s=torch.tensor(t["s"]), r=torch.tensor(t["r"]), o=torch.tensor(t["o"]),
                  z=torch.tensor(t["z"]), act=torch.tensor(opacities(CASE_P, seed)), raw_o=torch.tensor(raw_o),
                  raw_s=torch.tensor(raw_s), counts=torch.tensor(counts), rows=torch.tensor(rows),
                  wide=torch.tensor(t["xyz"]).repeat(1, 15), bits=torch.zeros(CASE_P, 4, dtype=torch.int32))


def _call_bits(t):
    return [_C().mcmc_random_bits(t["bits"], (1 << 40) + 3, 5, 2)]


def _call_sample(t):
    return list(_C().mcmc_sample(t["act"], MIN_O, 3000, (1 << 40) + 3, 5, 1))


def _call_relocate(t):
    _C().mcmc_relocate(t["raw_o"], t["raw_s"], t["counts"], MIN_O)
    return [t["raw_o"], t["raw_s"]]


def _call_noise(t):
    given = t["xyz"].clone()
    _C().mcmc_noise(t["xyz"], t["s"], t["r"], t["o"], 2.5, (1 << 40) + 3, 5, None)
    _C().mcmc_noise(given, t["s"], t["r"], t["o"], 2.5, 0, 0, t["z"])
    return [t["xyz"], given]


def _call_reg(t):
    go, gs = t["z"][:, :1].contiguous(), t["xyz"]
    return [_C().mcmc_reg_grad(t["o"], t["s"], 0.01, 0.02, go, gs), go, gs]


def _call_zero(t):
    _C().mcmc_zero_rows([t["xyz"], t["wide"], t["r"]], t["rows"])
    return [t["xyz"], t["wide"], t["r"]]


STREAM_CASES = [SC.Case(name, (name,), _case_inputs, call) for name, call in (
    ("mcmc_random_bits", _call_bits), ("mcmc_sample", _call_sample), ("mcmc_relocate", _call_relocate),
    ("mcmc_noise", _call_noise), ("mcmc_reg_grad", _call_reg), ("mcmc_zero_rows", _call_zero))]


def test_every_bound_entry_has_a_stream_case():
    import re
    with open(os.path.join(SC.CSRC, "mcmc_glue.cpp")) as f:
        bound = re.findall(r'm\.def\(\s*"(\w+)"', f.read())
    assert sorted(bound) == sorted(c.name for c in STREAM_CASES) and len(bound) == 6


@pytest.fixture(scope="module")
def side_streams():
    cal = SC.calibration(DEV)
    first = cal.fresh_stream()
    return first, cal.fresh_stream(apart_from=(first,))


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_entry_on_a_side_stream(side_streams, case):
    SC.run_case(case, side_streams[0], probe_stream=side_streams[1])


two_devices = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU (one device visible)")


@two_devices
@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_entry_on_the_second_device(case):
    """device 0 current, no device context: the outputs live on cuda:1 and hold device 0's bytes"""
    assert torch.cuda.current_device() == 0
    want = SC.run_default(case, SC.to_device(case.make(SC.SEED), "cuda:0"))
    got = [o.detach() for o in case.call(SC.to_device(case.make(SC.SEED), "cuda:1"))]
    assert torch.cuda.current_device() == 0 and all(o.device == torch.device("cuda:1") for o in got)
    torch.cuda.synchronize("cuda:1")
    assert SC.first_difference(got, want) is None
