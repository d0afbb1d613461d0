"""GPU tests of the blend backward's pair reduction (render.hip wave_sum_pair_to_lds) through the diagnostic
gs4d_debug_wave_sum, which reduces given per-lane partial sums of n pairs of splats to their two 12-float records
twice: by column sums through LDS (the blend kernel's form) and by v_permlane32_swap / v_permlane16_swap (the form it
replaced, kept as this comparison's reference).  Both add the four lanes of a column as (row 0 + row 2) + (row 1 +
row 3), so the records must agree bit for bit in all four (DEPTH, ABS) instantiations; inputs whose magnitudes span
2^-20 .. 2^20 with mixed signs make any other association show.

Independently of the permlane form, every record value is also compared with its fp64 sum: an fp32 sum of 64 terms
in any order is within 64 eps32 sum|terms| of it (the dx-weighted ones carry up to three more roundings per term: 70).

The resident workgroups per CU (gs4d_debug_backward_occupancy) must stay at 4 waves per SIMD -- 16 single-wave
workgroups -- for the colour and depth instantiations and 3 -- 12 -- for the two absgrad ones: the reduction's 1 KiB
of LDS must not cost a wave.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (depth, abs)
IDS = ["color", "depth", "abs", "depth+abs"]
N_PAIRS = 256
EPS32 = 2.0 ** -24


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def random_inputs(n, seed):
    """n x 20 x 64 float32: magnitudes 2^-20 .. 2^20 (log-uniform), random signs; the two dx rows (18, 19) are
    constant down each lane column, as a pixel column's mean.x - pixel x is"""
    g = torch.Generator().manual_seed(seed)
    x = torch.exp2(torch.rand(n, 20, 64, generator=g, dtype=torch.float64) * 40.0 - 20.0)
    x = torch.where(torch.rand(n, 20, 64, generator=g) < 0.5, -x, x).float()
    x[:, 18:20, :] = x[:, 18:20, :16].repeat(1, 1, 4)
    return x


def written(depth, absg):
    """which of a record's 12 floats the instantiation produces"""
    m = np.zeros(12, bool)
    m[:9] = True
    m[9] = depth
    m[10:] = absg
    return np.concatenate([m, m])


def fp64_records(x):
    """(the records' fp64 values, the sums of their terms' magnitudes), each n x 24, from the inputs n x 20 x 64"""
    x = x.double()
    out, mag = [], []
    for k0, w3, ax, dx in ((0, 12, 14, 18), (6, 13, 16, 19)):
        u0, u1, u2, w0, w1, w2 = (x[:, k0 + i] for i in range(6))
        d = x[:, dx]
        terms = [u0, d * u0, u1, d * d * u0, d * u1, u2, w0, w1, w2, x[:, w3], x[:, ax], x[:, ax + 1]]
        out += [t.sum(1) for t in terms]
        mag += [t.abs().sum(1) for t in terms]
    return torch.stack(out, 1).numpy(), torch.stack(mag, 1).numpy()


def run(x, depth, absg):
    lds, perm = _C().debug_wave_sum(x.cuda(), depth, absg)
    torch.cuda.synchronize()
    assert lds.shape == perm.shape == (x.shape[0], 24)
    return lds.cpu(), perm.cpu()


@pytest.mark.parametrize("depth,absg", VARIANTS, ids=IDS)
def test_lds_column_sums_equal_permlane_sums_bitwise(depth, absg):
    x = random_inputs(N_PAIRS, seed=7 + 2 * depth + absg)
    lds, perm = run(x, depth, absg)
    assert torch.equal(lds, perm), f"{int((lds != perm).sum())} record floats differ"
    m = written(depth, absg)
    mt = torch.from_numpy(m)
    assert not lds[:, ~mt].any(), "a float the instantiation does not produce was written"
    assert (lds[:, mt] != 0).all()
    want, mag = fp64_records(x)
    err = np.abs(lds.numpy().astype(np.float64) - want)[:, m] / (70 * EPS32 * mag[:, m])
    print(f"[wave-sum] depth={depth} abs={absg}: worst |fp32 - fp64| / (70 eps sum|terms|) = {err.max():.3f}",
          flush=True)
    assert err.max() <= 1.0


@pytest.mark.parametrize("depth,absg", VARIANTS, ids=IDS)
def test_zero_inputs_give_zero_records(depth, absg):
    lds, perm = run(torch.zeros(3, 20, 64), depth, absg)
    assert torch.equal(lds, perm) and not lds.any()


@pytest.mark.parametrize("depth,absg", VARIANTS, ids=IDS)
def test_single_lane_lands_in_its_record_floats(depth, absg):
    """one pair per lane of (0, 15, 16, 31, 32, 63): only that lane's sums are non-zero (dx is set in its whole
    column), so every record float is that lane's own value, exactly"""
    lanes = [0, 15, 16, 31, 32, 63]
    src = random_inputs(len(lanes), seed=31)
    x = torch.zeros_like(src)
    for i, l in enumerate(lanes):
        x[i, :18, l] = src[i, :18, l]
        x[i, 18:, l % 16::16] = src[i, 18:, l % 16::16]
    lds, perm = run(x, depth, absg)
    assert torch.equal(lds, perm)
    m = written(depth, absg)
    for i, l in enumerate(lanes):
        v = x[i, :, l]
        want = []
        for k0, w3, ax, dx in ((0, 12, 14, 18), (6, 13, 16, 19)):
            d = v[dx]
            want += [v[k0], v[k0] * d, v[k0 + 1], (v[k0] * d) * d, v[k0 + 1] * d, v[k0 + 2], v[k0 + 3], v[k0 + 4],
                     v[k0 + 5], v[w3], v[ax], v[ax + 1]]
        want = torch.stack(want) * torch.from_numpy(m).float()
        assert torch.equal(lds[i], want), (l, lds[i], want)


def test_backward_keeps_its_waves_per_simd():
    occ = {i: _C().debug_backward_occupancy(d, a) for i, (d, a) in zip(IDS, VARIANTS)}
    print(f"[wave-sum] resident workgroups per CU: {occ}", flush=True)
    assert occ["color"] >= 16 and occ["depth"] >= 16
    assert occ["abs"] >= 12 and occ["depth+abs"] >= 12
