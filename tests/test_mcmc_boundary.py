"""MCMC densification without a GPU: the generator's known answers and statistics, the correction formula against an
independent restatement, the C ABI's declarations, exports and status codes (through ctypes: every refusal comes
before any launch), the CPU formulation of relocate / grow on a small model, and train_step's schedule."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mcmc_refs as MR
from mcmc_models import PARAM_ATTRS, make_model, moments, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
OK, ERR_ARG, ERR_ALLOC = 0, 1, 2
ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
NULL_ALLOC = ctypes.cast(None, ALLOC_FN)
PTR = 0x1000  # a non-NULL pointer that is never dereferenced: the refusals come before any launch
ENTRIES = ("gs4d_mcmc_random_bits", "gs4d_mcmc_sample", "gs4d_mcmc_relocate", "gs4d_mcmc_noise", "gs4d_mcmc_reg_grad",
           "gs4d_mcmc_zero_rows")


# ---- the generator ----------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    """Random123's three philox4x32-10 vectors"""
    assert " ".join("%08x" % w for w in MR.philox4x32_10(counter, key)) == want


def test_the_numpy_generator_is_the_reference():
    from gs4d_train import mcmc
    for n, seed, it, purpose in ((0, 0, 0, 0), (1, 0, 1, 0), (300, (5 << 32) + 7, 9, 2), (65, 2 ** 64 - 1, 2 ** 32 - 1, 1)):
        got = mcmc.philox_words(n, seed, it, purpose)
        assert got.dtype == np.uint32 and got.shape == (n, 4) and np.array_equal(got, MR.blocks(n, seed, it, purpose))
    # the key is (seed lo, seed hi), the counter (j, purpose, iteration, 0)
    assert tuple(MR.blocks(4, (9 << 32) | 8, 6, 2)[3]) == MR.philox4x32_10((3, 2, 6, 0), (8, 9))


def test_normal_statistics():
    from gs4d_train import mcmc
    P = 65536
    z = MR.normals64(mcmc.philox_words(P, 0, 1, MR.NOISE))
    N = 3 * P
    mean, var = abs(float(z.mean())), abs(float(z.var()) - 1.0)
    print(f"[mcmc] normals: |mean| {mean:.2e} (bar {5 / math.sqrt(N):.2e}), |var - 1| {var:.2e} "
          f"(bar {5 * math.sqrt(2 / N):.2e})")
    assert mean < 5 / math.sqrt(N) and var < 5 * math.sqrt(2 / N)
    e32 = float(np.abs(mcmc.normals_numpy(P, 0, 1).astype(np.float64) - z).max())
    print(f"[mcmc] numpy-fp32 Box-Muller against fp64: {e32:.2e} absolute")
    assert e32 < 1e-3 and np.isfinite(z).all()


# ---- the correction ---------------------------------------------------------------------------------------------------
def _restated(o, n):
    """(o', s'/s) another way: o' as the textbook 1 - (1 - o)^(1/n) in 50-digit decimal arithmetic, D by the
    hockey-stick identity sum_{i=k+1..n} C(i-1, k) = C(n, k+1), its terms in decimal too"""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        od = decimal.Decimal(o)
        o_new = 1 - (1 - od) ** (decimal.Decimal(1) / n)
        total = sum(decimal.Decimal(math.comb(n, k + 1) * (-1) ** k) * o_new ** (k + 1) / decimal.Decimal(k + 1).sqrt()
                    for k in range(n))
        return float(o_new), float(od / total)


def test_relocation_formula():
    for o in (0.005, 0.3, 0.9, 0.999):
        o1, r1 = MR.relocated(o, 1)
        assert abs(o1 - o) <= 1e-15 and abs(r1 - 1.0) <= 1e-15  # n = 1: the identity
        for n in (2, 5, 51):
            got, want = MR.relocated(o, n), _restated(o, n)
            print(f"[mcmc] o {o} n {n}: o' {got[0]:.12g} s'/s {got[1]:.12g}")
            assert abs(got[0] - want[0]) <= 1e-14 * want[0]
            assert abs(got[1] - want[1]) <= 1e-9 * want[1]  # the fp64 alternating sum loses digits to cancellation at n = 51
            assert abs((1 - got[0]) ** n - (1 - o)) <= 1e-12  # n copies of o' hide what one of o hid
            assert 0.5 < got[1] < 1.0  # the copies shrink
    # the textbook form loses digits in fp32 where the expm1 / log1p form does not
    o, n = np.float32(0.005), 51
    exact = MR.relocated(float(o), n)[0]
    textbook = float(np.float32(1) - np.power(np.float32(1) - o, np.float32(1 / n)))
    stable = float(-np.expm1(np.log1p(-o) / np.float32(n)))
    print(f"[mcmc] fp32 o' at o = 0.005, n = 51: textbook off by {abs(textbook - exact) / exact:.1e}, "
          f"expm1 / log1p by {abs(stable - exact) / exact:.1e}")
    assert abs(stable - exact) < 1e-6 * exact and abs(textbook - exact) > 1e-5 * exact


def test_the_torch_correction_is_the_reference():
    from gs4d_train import mcmc
    rng = np.random.default_rng(3)
    P = 64
    o = rng.uniform(0.0051, 0.999, P)
    o[:4] = (0.0050001, 0.3, 0.9, 0.999)
    raw_o = torch.tensor(np.log(o / (1 - o)), dtype=torch.float32).reshape(P, 1)
    raw_s = torch.tensor(rng.normal(-3, 1, (P, 3)), dtype=torch.float32)
    counts = torch.tensor(rng.integers(0, 4, P), dtype=torch.int32)
    counts[:4] = torch.tensor([60, 50, 1, 4], dtype=torch.int32)
    rows, new_o, new_s = mcmc.corrected_torch(raw_o, raw_s, counts, 0.005)
    want_o, want_s = MR.relocate_rows(raw_o.numpy(), raw_s.numpy(), counts.numpy(), 0.005)
    assert np.array_equal(rows.numpy(), np.nonzero(counts.numpy() > 0)[0])
    e_o = np.abs(new_o.numpy().astype(np.float64) - want_o[rows.numpy()]).max() / np.abs(want_o).max()
    e_s = np.abs(new_s.numpy().astype(np.float64) - want_s[rows.numpy()]).max() / np.abs(want_s).max()
    print(f"[mcmc] torch fp32 correction against fp64: opacity {e_o:.2e}, scaling {e_s:.2e}")
    assert e_o < 1e-5 and e_s < 1e-5


# ---- the sampler ------------------------------------------------------------------------------------------------------
def test_the_numpy_sampler_is_the_reference():
    from gs4d_train import mcmc
    rng = np.random.default_rng(0)
    o = rng.random(1000).astype(np.float32)
    o[::3] = 0.001
    cases = [(o, 700), (o, 0), (o[:1], 5), (np.full(50, 0.004, np.float32), 9), (np.full(77, 0.25, np.float32), 300),
             (np.concatenate([np.full(30, 0.006, np.float32), [np.float32(1 - 2.0 ** -24)]]), 200)]
    for op, n in cases:
        got, want = mcmc.sample_numpy(op, 0.005, n, 3, 4, MR.RELOCATE), MR.sample(op, 0.005, n, 3, 4, MR.RELOCATE)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and int(got[1].sum()) == got[2]
        assert not (got[1][op <= np.float32(0.005)] != 0).any()  # a dead row is never drawn
    assert mcmc.sample_numpy(cases[3][0], 0.005, 9, 3, 4, 1)[2] == 0  # no live row: zero draws
    heavy = mcmc.sample_numpy(cases[5][0], 0.005, 2000, 1, 2, 2)[1]
    assert 0.7 < heavy[-1] / 2000 < 0.95  # 1 / (1 + 30 * 0.006) = 0.85 of the weight


# ---- headers, exports, status codes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    p, i, f, u64, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32
    L.gs4d_mcmc_random_bits.argtypes = [i, u64, u32, u32, p, p]
    L.gs4d_mcmc_sample.argtypes = [i, p, f, i, u64, u32, u32, p, p, p, ALLOC_FN, p, p]
    L.gs4d_mcmc_relocate.argtypes = [i, p, f, p, p, p]
    L.gs4d_mcmc_noise.argtypes = [i, p, p, p, p, f, u64, u32, p, p]
    L.gs4d_mcmc_reg_grad.argtypes = [i, p, p, f, f, p, p, p, ALLOC_FN, p, p]
    L.gs4d_mcmc_zero_rows.argtypes = [p, p]
    return L


class Allocator:
    """counts its calls and returns NULL"""

    def __init__(self):
        self.calls = 0
        self.fn = ALLOC_FN(self._alloc)

    def _alloc(self, ctx, n):
        self.calls += 1
        return None


def test_headers_declare_the_entries():
    with open(os.path.join(ROOT, "include", "gs4d_train.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
    assert "GS4D_MCMC_NOISE = 0, GS4D_MCMC_RELOCATE = 1, GS4D_MCMC_GROW = 2" in text


def test_library_exports_the_entries(lib):
    for name in ENTRIES:
        assert getattr(lib, name), name


def _refused(lib, status):
    assert status == ERR_ARG and lib.gs4d_last_error().startswith(b"mcmc:"), (status, lib.gs4d_last_error())


def test_status_codes(lib):
    a = Allocator()
    bits = lambda n, out=PTR: lib.gs4d_mcmc_random_bits(n, 1, 2, 0, out, None)
    assert bits(0) == OK and bits(0, None) == OK
    _refused(lib, bits(-1))
    _refused(lib, bits(5, None))

    def sample(P, n, alloc, o=PTR, draws=PTR, counts=PTR, m=0.005):
        return lib.gs4d_mcmc_sample(P, o, m, n, 1, 2, 1, draws, counts, None, alloc, None, None)
    assert sample(0, 7, a.fn) == OK and sample(100, 0, a.fn) == OK and sample(0, 0, NULL_ALLOC, None, None, None) == OK
    for P, n in ((-1, 5), (100, -1)):
        _refused(lib, sample(P, n, a.fn))
    _refused(lib, sample(100, 5, a.fn, m=-0.1))
    _refused(lib, sample(100, 5, a.fn, m=float("nan")))
    _refused(lib, sample(100, 5, NULL_ALLOC))
    for name in ("o", "draws", "counts"):
        _refused(lib, sample(100, 5, a.fn, **{name: None}))
    assert a.calls == 0  # every refusal above came before the allocator was asked
    assert sample(100, 5, a.fn) == ERR_ALLOC and lib.gs4d_last_error().startswith(b"mcmc:") and a.calls == 1

    def relocate(P, counts=PTR, o=PTR, s=PTR, m=0.005):
        return lib.gs4d_mcmc_relocate(P, counts, m, o, s, None)
    assert relocate(0) == OK
    _refused(lib, relocate(-1))
    for m in (0.0, 1.0, -1.0, float("nan")):
        _refused(lib, relocate(100, m=m))
    for name in ("counts", "o", "s"):
        _refused(lib, relocate(100, **{name: None}))

    def noise(P, xyz=PTR, s=PTR, r=PTR, o=PTR):
        return lib.gs4d_mcmc_noise(P, xyz, s, r, o, 1.0, 1, 2, None, None)
    assert noise(0) == OK
    _refused(lib, noise(-1))
    for name in ("xyz", "s", "r", "o"):
        _refused(lib, noise(100, **{name: None}))

    b = Allocator()

    def reg(P, alloc, o=PTR, s=PTR, value=PTR):
        return lib.gs4d_mcmc_reg_grad(P, o, s, 0.01, 0.01, value, None, None, alloc, None, None)
    assert reg(0, b.fn) == OK
    _refused(lib, reg(-1, b.fn))
    _refused(lib, reg(100, NULL_ALLOC))
    for name in ("o", "s", "value"):
        _refused(lib, reg(100, b.fn, **{name: None}))
    assert b.calls == 0
    assert reg(100, b.fn) == ERR_ALLOC and lib.gs4d_last_error().startswith(b"mcmc:") and b.calls == 1


class _ZeroTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_int64)]


class _ZeroBatch(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int), ("P", ctypes.c_int64), ("n", ctypes.c_int64), ("rows", ctypes.c_void_p),
                ("t", _ZeroTensor * 32)]


def test_zero_rows_status_codes(lib):
    def call(count=2, P=100, n=5, rows=PTR, data=PTR, width=3):
        b = _ZeroBatch(count=count, P=P, n=n, rows=rows)
        for i in range(max(0, min(count, 32))):
            b.t[i] = _ZeroTensor(data, width)
        return lib.gs4d_mcmc_zero_rows(ctypes.byref(b), None)
    _refused(lib, lib.gs4d_mcmc_zero_rows(None, None))
    assert call(count=0) == OK and call(n=0) == OK and call(P=0) == OK
    for kw in (dict(count=-1), dict(count=33), dict(P=-1), dict(n=-1), dict(rows=None), dict(data=None), dict(width=0)):
        _refused(lib, call(**kw))


# ---- relocate / grow on a CPU model ----------------------------------------------------------------------------------
MIN_O = 0.005


def test_relocate_on_a_cpu_model():
    from gs4d_train import mcmc
    dead = (3, 4, 17, 30, 39)
    g, _, _ = make_model(dead=dead)
    before = snapshot(g)
    assert len(before["moments"]) == 12 and all(float(m.abs().min()) > 0 for m in before["moments"][:2])
    opacity = g.get_opacity.detach().reshape(-1).numpy()
    draws, counts, drawn = MR.sample(opacity, MIN_O, len(dead), 11, 700, MR.RELOCATE)
    assert drawn == len(dead) and not set(draws.tolist()) & set(dead)
    gen = g.row_generation if hasattr(g, "row_generation") else 0
    assert mcmc.relocate(g, 11, 700, MIN_O) == len(dead)
    after = snapshot(g)
    assert g.row_generation == gen + 1 and after["_xyz"].shape[0] == 40
    # the sources were corrected (the reference's values), then copied
    want_o, want_s = MR.relocate_rows(before["_opacity"].numpy(), before["_scaling"].numpy(), counts, MIN_O)
    sources = sorted(set(draws.tolist()))
    for r in sources:
        assert abs(float(after["_opacity"][r]) - want_o[r, 0]) <= 1e-5 * abs(want_o).max()
        assert np.abs(after["_scaling"][r].numpy() - want_s[r]).max() <= 1e-5 * abs(want_s).max()
    for j, d in enumerate(dead):  # the j-th dead row is a copy of row draws[j]
        for a in PARAM_ATTRS:
            assert torch.equal(after[a][d], after[a][int(draws[j])]), (a, d)
        assert bool(after["table"][d]) == bool(before["table"][int(draws[j])])
        assert all(float(s[d].abs().sum()) == 0 for s in after["stats"])
    touched = sorted(set(dead) | set(sources))
    others = [r for r in range(40) if r not in touched]
    for m0, m1 in zip(before["moments"], after["moments"]):
        assert float(m1[touched].abs().sum()) == 0 and torch.equal(m1[others], m0[others])
    for a in PARAM_ATTRS:
        assert torch.equal(after[a][others], before[a][others]), a
    for a in ("_xyz", "_features_dc", "_features_rest", "_rotation"):  # a source keeps all but opacity and scale
        assert torch.equal(after[a][sources], before[a][sources]), a
    live_stats = [r for r in range(40) if r not in dead]
    for s0, s1 in zip(before["stats"], after["stats"]):
        assert torch.equal(s1[live_stats], s0[live_stats])
    # a source clamped to min_opacity is stored as logit(min_opacity), whose fp32 sigmoid may land an ulp below it
    assert float(g.get_opacity.detach().min()) > 0.9 * MIN_O and g._opacity.requires_grad and g._opacity.grad is None


@pytest.mark.parametrize("dead", [(), tuple(range(40))], ids=["none dead", "all dead"])
def test_relocate_is_a_no_op_without_dead_or_live_rows(dead):
    from gs4d_train import mcmc
    g, _, _ = make_model(dead=dead)
    if not dead:
        with torch.no_grad():
            g._opacity.clamp_(min=-3.0)
    before, gen = snapshot(g), getattr(g, "row_generation", 0)
    params = [getattr(g, a) for a in PARAM_ATTRS]
    assert mcmc.relocate(g, 11, 700, MIN_O) == 0
    after = snapshot(g)
    assert getattr(g, "row_generation", 0) == gen and all(getattr(g, a) is p for a, p in zip(PARAM_ATTRS, params))
    for a in PARAM_ATTRS:
        assert torch.equal(after[a], before[a])
    assert all(torch.equal(x, y) for x, y in zip(after["moments"] + after["stats"], before["moments"] + before["stats"]))
    if dead:  # nothing to draw from: growth is a no-op too
        assert mcmc.grow(g, 11, 700, 1000, MIN_O) == 0 and g._xyz.shape[0] == 40


@pytest.mark.parametrize("cap,want", [(1000, 42), (41, 41), (40, 40), (30, 40)])
def test_grow_on_a_cpu_model(cap, want):
    from gs4d_train import mcmc
    g, _, _ = make_model()
    before = snapshot(g)
    n_new = want - 40
    assert int(1.05 * 40) == 42
    opacity = g.get_opacity.detach().reshape(-1).numpy()
    draws, counts, _ = MR.sample(opacity, MIN_O, n_new, 5, 900, MR.GROW)
    assert mcmc.grow(g, 5, 900, cap, MIN_O) == n_new
    after = snapshot(g)
    assert after["_xyz"].shape[0] == want == min(max(cap, 40), int(1.05 * 40))
    if n_new == 0:
        assert all(torch.equal(after[a], before[a]) for a in PARAM_ATTRS)
        return
    sources = sorted(set(draws.tolist()))
    others = [r for r in range(40) if r not in sources]
    for j in range(n_new):
        for a in PARAM_ATTRS:
            assert torch.equal(after[a][40 + j], after[a][int(draws[j])]), (a, j)
        assert bool(after["table"][40 + j]) == bool(before["table"][int(draws[j])])
    want_o, _ = MR.relocate_rows(before["_opacity"].numpy(), before["_scaling"].numpy(), counts, MIN_O)
    for r in sources:
        assert abs(float(after["_opacity"][r]) - want_o[r, 0]) <= 1e-5 * abs(want_o).max()
    for m0, m1 in zip(before["moments"], after["moments"]):
        assert m1.shape[0] == want and float(m1[sources + list(range(40, want))].abs().sum()) == 0
        assert torch.equal(m1[others], m0[others])
    for s0, s1 in zip(before["stats"], after["stats"]):
        assert torch.equal(s1[:40], s0) and float(s1[40:].abs().sum()) == 0
    for a in PARAM_ATTRS:
        assert torch.equal(after[a][others], before[a][others]), a


def test_noise_and_regulariser_cpu_formulations():
    from gs4d_train import mcmc
    g, _, _ = make_model(stepped=False)
    with torch.no_grad():
        g._opacity[0] = 7.0  # opacity 0.999: gated
    x0 = g._xyz.detach().clone()
    mcmc.inject_noise(g, 0.3, 21, 5)
    words = MR.blocks(40, 21, 5, MR.NOISE)
    want = MR.noise_delta(g._scaling.detach().numpy(), g._rotation.detach().numpy(), g._opacity.detach().numpy(), 0.3,
                          MR.normals64(words))
    got = (g._xyz.detach() - x0).numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max() and np.abs(want).max() > 0
    assert np.abs(got[0]).max() < 1e-30 * float(np.exp(g._scaling.detach().numpy()[0]).max())
    x1 = g._xyz.detach().clone()
    given = torch.randn(40, 3, generator=torch.Generator().manual_seed(1))
    mcmc.inject_noise(g, 0.3, 21, 5, normals=given)
    want = MR.noise_delta(g._scaling.detach().numpy(), g._rotation.detach().numpy(), g._opacity.detach().numpy(), 0.3,
                          given.numpy())
    assert np.abs((g._xyz.detach() - x1).numpy() - want).max() <= 1e-4 * np.abs(want).max()
    # the regulariser: value, and gradients ADDED to what the buffers hold
    g._opacity.grad = torch.full_like(g._opacity, 0.5)
    value = mcmc.regulariser_and_grad(g, 0.01, 0.02)
    v, go, gs = MR.regulariser(g._opacity.detach().numpy(), g._scaling.detach().numpy(), 0.01, 0.02)
    assert abs(float(value) - v) <= 1e-6 * abs(v) and not value.requires_grad
    assert np.abs(g._opacity.grad.numpy() - (0.5 + go)).max() <= 1e-6
    assert np.abs(g._scaling.grad.numpy() - gs).max() <= 1e-6 * np.abs(gs).max()


# ---- train_step's schedule --------------------------------------------------------------------------------------------
H = W = 6


def make_views(n):
    gen = torch.Generator().manual_seed(7)
    return [(SimpleNamespace(A=torch.randn(3, 2, generator=gen) + 2.0, time=i / max(n, 1)), torch.rand(3, H, W, generator=gen))
            for i in range(n)]


def splat_render(cam, pc, debug, bg, stage="coarse"):
    """render()'s dict from a differentiable isotropic splatter (tests/test_train_dp_gloo.py's stand-in)"""
    xyz = pc.get_xyz
    ss = torch.zeros_like(xyz, requires_grad=True) + 0
    ss.retain_grad()
    m2 = xyz @ cam.A + ss[:, :2]
    s = pc.get_scaling.max(dim=1).values * 20
    op = pc.get_opacity[:, 0]
    col = pc.get_features[:, 0, :] * 0.28 + 0.5
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xx.reshape(-1), yy.reshape(-1)], 1)
    vis = xyz[:, 2] > 0
    wgt = (op * vis)[:, None] * torch.exp(-((pix[None] - m2[:, None]) ** 2).sum(-1) / (2 * s[:, None] ** 2 + 1))
    img = (wgt[:, :, None] * col[:, None, :]).sum(0) / (1 + wgt.sum(0)[:, None])
    radii = (torch.ceil(3 * s).to(torch.int32) * vis).to(torch.int32)
    return {"render": img.t().reshape(3, H, W), "viewspace_points": ss, "visibility_filter": radii > 0, "radii": radii,
            "depth": torch.zeros(1, H, W)}


def test_config_defaults():
    from gs4d_train import config
    opt = config.optimization_params()
    assert (opt.densify_strategy, opt.mcmc_cap_max, opt.mcmc_noise_lr, opt.mcmc_opacity_reg, opt.mcmc_scale_reg,
            opt.mcmc_min_opacity, opt.mcmc_seed) == ("default", 1_000_000, 5e5, 0.01, 0.01, 0.005, 0)


def test_train_step_schedule(monkeypatch):
    from gs4d_train import mcmc
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.train import train_step
    g, hyper, opt = make_model(stepped=False)
    opt.densify_strategy = "mcmc"
    opt.densify_from_iter, opt.densify_until_iter, opt.densification_interval = 4, 12, 3
    opt.opacity_reset_interval, opt.mcmc_seed = 5, 77
    calls = []
    for name in ("relocate", "grow", "inject_noise", "regulariser_and_grad"):
        def spy(*a, _f=getattr(mcmc, name), _n=name, **kw):
            calls.append((_n, a[1:], kw))
            return _f(*a, **kw)
        monkeypatch.setattr(mcmc, name, spy)
    for name in ("reset_opacity", "densify", "prune", "add_densification_stats"):
        def banned(self, *a, _n=name, **kw):
            raise AssertionError(f"{_n} called with densify_strategy = \"mcmc\"")
        monkeypatch.setattr(GaussianModel, name, banned)
    views, bg = make_views(1), torch.ones(3)
    fired, P = [], [g._xyz.shape[0]]
    for it in range(1, 15):
        calls.clear()
        loss = train_step(g, views, opt, hyper, it, bg, stage="coarse", render_fn=splat_render)
        names = [c[0] for c in calls]
        xyz_lr = next(q["lr"] for q in g.optimizer.param_groups if q["name"] == "xyz")
        assert names[0] == "regulariser_and_grad" and names[-1] == "inject_noise" and torch.isfinite(loss)
        step_scale, seed, iteration = calls[-1][1]
        assert (seed, iteration) == (77, it) and abs(step_scale - opt.mcmc_noise_lr * xyz_lr) <= 1e-12 * step_scale
        if "relocate" in names:
            assert names == ["regulariser_and_grad", "relocate", "grow", "inject_noise"]
            assert calls[1][1] == (77, it, opt.mcmc_min_opacity)
            assert calls[2][1] == (77, it, opt.mcmc_cap_max, opt.mcmc_min_opacity)
            fired.append(it)
        else:
            assert names == ["regulariser_and_grad", "inject_noise"]
        P.append(g._xyz.shape[0])
    assert fired == [6, 9]  # 4 < it < 12 and it % 3 == 0
    assert P[6] == int(1.05 * P[5]) and P[9] == int(1.05 * P[8]) and P[-1] == P[9] > P[0]
    assert float(g.get_opacity.detach().min()) > 0.9 * opt.mcmc_min_opacity  # the dead rows were relocated


def test_train_step_loss_carries_the_regulariser_and_default_is_unchanged():
    from gs4d_train.train import train_step
    views, bg = make_views(1), torch.ones(3)
    out = {}
    for strategy in ("absent", "default", "mcmc"):
        g, hyper, opt = make_model(stepped=False)
        if strategy == "absent":  # an opt built before the option existed
            for k in [k for k in vars(opt) if k.startswith("mcmc_") or k == "densify_strategy"]:
                delattr(opt, k)
        else:
            opt.densify_strategy = strategy
        opt.mcmc_noise_lr = 0.0 if strategy == "mcmc" else 5e5
        reg = MR.regulariser(g._opacity.detach().numpy(), g._scaling.detach().numpy(), 0.01, 0.01)[0]
        loss = train_step(g, views, opt, hyper, 3, bg, stage="coarse", render_fn=splat_render)
        out[strategy] = (float(loss), snapshot(g), reg)
    for a in PARAM_ATTRS:
        assert torch.equal(out["absent"][1][a], out["default"][1][a]), a
    assert out["absent"][0] == out["default"][0]
    assert abs(out["mcmc"][0] - (out["default"][0] + out["mcmc"][2])) <= 1e-6 * abs(out["mcmc"][0])
    assert not torch.equal(out["mcmc"][1]["_opacity"], out["default"][1]["_opacity"])  # its gradient reached the step
    g, hyper, opt = make_model(stepped=False)
    opt.densify_strategy = "metropolis"
    with pytest.raises(ValueError):
        train_step(g, views, opt, hyper, 3, bg, stage="coarse", render_fn=splat_render)
