"""MCMC densification (opt-in; 3DGS-MCMC, Kheradmand et al. 2024; gsplat's MCMCStrategy is the model; the reference
has no counterpart): relocation of dead Gaussians, growth to a budget, per-step position noise and the opacity /
scale regulariser.

    relocate   the dead rows (opacity <= min_opacity), in ascending order, become copies of live rows drawn with
               replacement in proportion to opacity; a source drawn c times has its opacity and scale corrected for
               n = min(c + 1, 51) copies so that the rendered image does not change:
                   o' = 1 - (1 - o)^(1/n),   s' = s o / D,
                   D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1).
    grow       min(cap_max, int(growth P)) - P further copies, drawn and corrected the same way, are appended.
    noise      every step: x += R diag(s^2) R^T (z g step_scale), z standard normals,
               g = 1 / (1 + exp(-100 ((1 - o) - 0.995))) (opaque Gaussians stay put).
    regulariser  w_opacity mean(o) + w_scale mean(s), its gradient added to the parameters' .grad.

Every random number is a word of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
(j, purpose, iteration, 0) -- j the row or draw index, purpose 0 noise / 1 relocation / 2 growth -- so the draws are a
function of (seed, iteration) alone: two processes, or the replicas of a data-parallel step, make the same ones with
no collective.  The sampler is exact and order-free: integer weights (u64)(o 2^32), 64-bit inclusive prefix sums S,
t = (u S[P-1]) >> 64 for u = w0 | w1 << 32 of block d, the first row with S[i] > t.

With `gaussians.fused` on a GPU each function runs the HIP kernels of csrc/mcmc.hip (one launch for the noise, one
for the correction, four for a sampling, one for all the moments' rows).  Otherwise -- fused=False, or CPU tensors --
the torch / numpy formulations below run: the same draws bit for bit (numpy uint64 Philox and prefix sums), the
arithmetic in torch fp32 (the correction's D in fp64).  They are what the GPU tests measure the kernels against.
Rows are moved by one surgery.RowPlan either way, so the deformation table and row_generation follow.
"""
import math

import numpy as np
import torch

from . import surgery

__all__ = ["relocate", "grow", "inject_noise", "regulariser_and_grad", "philox_words", "normals_numpy", "sample_numpy",
           "corrected_torch", "noise_delta_torch", "NOISE", "RELOCATE", "GROW", "N_MAX"]

NOISE, RELOCATE, GROW = 0, 1, 2  # the counter's purpose word (GS4D_MCMC_* of include/gs4d_train.h)
N_MAX = 51
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


# ---- the generator and the sampler in numpy ---------------------------------------------------------------------------
def philox_words(n, seed, iteration, purpose):
    """(n, 4) uint32: the words of Philox4x32-10 blocks 0 .. n - 1 (numpy uint64 arithmetic: a 32 x 32-bit product
    fits without wrapping)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = [np.arange(n, dtype=np.uint64), np.full(n, int(purpose) & 0xFFFFFFFF, np.uint64),
         np.full(n, int(iteration) & 0xFFFFFFFF, np.uint64), np.zeros(n, np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def normals_numpy(P, seed, iteration):
    """(P, 3) float32: the noise kernel's Box-Muller normals of blocks 0 .. P - 1, in numpy fp32"""
    w = philox_words(P, seed, iteration, NOISE)
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    r0 = np.sqrt(np.float32(-2.0) * np.log(u[:, 0]))
    r1 = np.sqrt(np.float32(-2.0) * np.log(u[:, 2]))
    two_pi = np.float32(2.0 * math.pi)
    return np.stack([r0 * np.cos(two_pi * u[:, 1]), r0 * np.sin(two_pi * u[:, 1]), r1 * np.cos(two_pi * u[:, 3])],
                    1).astype(np.float32)


def _mulhi64(u, t):
    """the high 64 bits of u * t (uint64 arrays / scalars) from 32-bit halves"""
    ul, uh, tl, th = u & _MASK, u >> _S32, t & _MASK, t >> _S32
    ll, lh, hl, hh = ul * tl, ul * th, uh * tl, uh * th
    mid = (ll >> _S32) + (lh & _MASK) + (hl & _MASK)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def sample_numpy(opacity, min_opacity, n, seed, iteration, purpose):
    """(draws (n) int32, counts (P) int32, drawn) for activated float32 opacities (P): gs4d_mcmc_sample's draws bit
    for bit.  drawn is n, or 0 when no row is live (draws and counts are then zeros)."""
    o = np.ascontiguousarray(opacity, dtype=np.float32).reshape(-1)
    P = o.shape[0]
    draws, counts = np.zeros(n, np.int32), np.zeros(P, np.int32)
    if P == 0 or n == 0:
        return draws, counts, 0
    live = o > np.float32(min_opacity)
    w = np.where(live, np.minimum(o, np.float32(1.0)).astype(np.float64) * 4294967296.0, 0.0).astype(np.uint64)
    S = np.cumsum(w, dtype=np.uint64)
    total = S[-1]
    if int(total) == 0:
        return draws, counts, 0
    words = philox_words(n, seed, iteration, purpose).astype(np.uint64)
    u = words[:, 0] | (words[:, 1] << _S32)
    t = _mulhi64(u, np.uint64(total))
    draws = np.searchsorted(S, t, side="right").astype(np.int32)  # the first i with S[i] > t
    counts = np.bincount(draws, minlength=P).astype(np.int32)
    return draws, counts, n


# ---- the torch formulations -----------------------------------------------------------------------------------------
_COEF = None


def _coefficients():
    """A[n, k] = sum_{i=k+1..n} C(i-1, k) (-1)^k / sqrt(k+1) (fp64), so that D = sum_k A[n, k] o'^(k+1)"""
    global _COEF
    if _COEF is None:
        A = np.zeros((N_MAX + 1, N_MAX), np.float64)
        for n in range(1, N_MAX + 1):
            A[n] = A[n - 1]
            for k in range(n):
                A[n, k] += math.comb(n - 1, k) * (-1.0) ** k / math.sqrt(k + 1)
        _COEF = torch.from_numpy(A)
    return _COEF


def corrected_torch(opacity_raw, scaling_raw, counts, min_opacity):
    """(rows, raw opacity', raw scaling') of the rows with counts > 0: gs4d_mcmc_relocate's values in torch fp32 (the
    denominator D in fp64, as the kernel's)"""
    rows = torch.nonzero(counts.reshape(-1) > 0).flatten()
    raw_o, raw_s = opacity_raw.detach()[rows].reshape(-1), scaling_raw.detach()[rows]
    n = torch.clamp(counts.reshape(-1)[rows].long() + 1, max=N_MAX)
    o = torch.sigmoid(raw_o)
    o_new = -torch.expm1(torch.log1p(-o) / n.to(o.dtype))
    A = _coefficients().to(o.device)[n]                                               # (rows, 51)
    powers = o_new.double()[:, None] ** torch.arange(1, N_MAX + 1, device=o.device, dtype=torch.float64)[None, :]
    D = (A * powers).sum(1)
    ratio = (o.double() / D).to(o.dtype)
    o_new = torch.clamp(o_new, min=float(np.float32(min_opacity)), max=float(np.float32(1.0) - np.float32(2.0 ** -23)))
    return rows, torch.log(o_new / (1 - o_new)).reshape(-1, *opacity_raw.shape[1:]), \
        torch.log(torch.exp(raw_s) * ratio[:, None])


def noise_delta_torch(scaling_raw, rotation_raw, opacity_raw, step_scale, normals):
    """the noise's position change in torch fp32: bmm(R S S^T R^T, z g step_scale), gsplat's formulation"""
    from .gaussians import build_rotation
    R = build_rotation(rotation_raw.detach())
    S = torch.diag_embed(torch.exp(scaling_raw.detach()))
    L = torch.bmm(R, S)
    cov = torch.bmm(L, L.transpose(1, 2))
    o = torch.sigmoid(opacity_raw.detach()).reshape(-1, 1)
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    noise = normals * gate * float(step_scale)
    return torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)


# ---- the public functions -------------------------------------------------------------------------------------------
def _fused(gaussians):
    return bool(getattr(gaussians, "fused", False)) and gaussians._xyz.is_cuda


def _seed(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _moments(gaussians):
    """the Adam moments of the per-Gaussian parameters (twelve tensors once the optimizer has stepped)"""
    opt = gaussians.optimizer
    out = []
    if opt is None:
        return out
    for g in opt.param_groups:
        if g["name"] in surgery.PARAMS:
            st = opt.state.get(g["params"][0])
            if st and "exp_avg" in st:
                out += [st["exp_avg"], st["exp_avg_sq"]]
    return out


def _zero_rows(gaussians, tensors, rows):
    """rows `rows` of every tensor zeroed in place: one launch for all of them on the fused path"""
    if not tensors or rows.numel() == 0:
        return
    if _fused(gaussians):
        from . import _C
        _C.mcmc_zero_rows([t for t in tensors], rows.to(torch.int32).contiguous())
    else:
        idx = rows.long()
        for t in tensors:
            t.index_fill_(0, idx, 0)


def _draw_and_correct(gaussians, opacity, n, seed, iteration, min_opacity, purpose):
    """n draws in proportion to opacity, and the drawn sources corrected in place; the draws (int32, on the model's
    device), or None when no row is live"""
    dev = gaussians._xyz.device
    if _fused(gaussians):
        from . import _C
        draws, counts, n_drawn = _C.mcmc_sample(opacity.contiguous(), float(min_opacity), int(n), _seed(seed),
                                                int(iteration), purpose)
        if int(n_drawn.item()) == 0:
            return None
        _C.mcmc_relocate(gaussians._opacity.data, gaussians._scaling.data, counts, float(min_opacity))
        return draws
    d, c, drawn = sample_numpy(opacity.detach().cpu().numpy(), min_opacity, int(n), _seed(seed), int(iteration), purpose)
    if drawn == 0:
        return None
    counts = torch.from_numpy(c).to(dev)
    rows, raw_o, raw_s = corrected_torch(gaussians._opacity, gaussians._scaling, counts, min_opacity)
    gaussians._opacity.data[rows] = raw_o
    gaussians._scaling.data[rows] = raw_s
    return torch.from_numpy(d).to(dev)


def relocate(gaussians, seed, iteration, min_opacity):
    """The dead rows (get_opacity <= min_opacity) in ascending order take the draws in draw order: the j-th dead row
    becomes a copy of row draws[j], after the sources' correction.  One row plan (a gather), then the statistics of
    the overwritten rows and the Adam moments of every source and destination row are zeroed.  A no-op when no row or
    every row is dead.  Returns the number of rows relocated."""
    with torch.no_grad():
        opacity = gaussians.get_opacity.detach().reshape(-1)
        P = opacity.shape[0]
        dead = torch.nonzero(opacity <= torch.tensor(float(min_opacity), dtype=opacity.dtype, device=opacity.device)).flatten()
        n_dead = int(dead.numel())
        if n_dead == 0 or n_dead == P:
            return 0
        draws = _draw_and_correct(gaussians, opacity, n_dead, seed, iteration, min_opacity, RELOCATE)
        if draws is None:
            return 0
        keep = torch.arange(P, device=opacity.device, dtype=torch.int64)
        keep[dead] = draws.to(torch.int64)
        surgery.apply(gaussians, surgery.RowPlan(keep=keep, n_new=0, stats="carry"))
        _zero_rows(gaussians, [getattr(gaussians, name) for name in surgery.STATS], dead)
        _zero_rows(gaussians, _moments(gaussians), torch.cat([dead.to(draws.dtype), draws]))
        return n_dead


def grow(gaussians, seed, iteration, cap_max, min_opacity, growth=1.05):
    """min(cap_max, int(growth P)) - P copies of rows drawn in proportion to opacity are appended (the sources
    corrected first); the moments of the sources and of the new rows are zero, the new rows' statistics too.
    Returns the number of rows added."""
    with torch.no_grad():
        P = gaussians._xyz.shape[0]
        n_new = min(int(cap_max), int(growth * P)) - P
        if n_new <= 0 or P == 0:
            return 0
        opacity = gaussians.get_opacity.detach().reshape(-1)
        draws = _draw_and_correct(gaussians, opacity, n_new, seed, iteration, min_opacity, GROW)
        if draws is None:
            return 0
        keep = torch.arange(P, device=opacity.device, dtype=torch.int64)
        surgery.apply(gaussians, surgery.RowPlan(keep=keep, append=draws, n_new=n_new, stats="carry"))
        _zero_rows(gaussians, _moments(gaussians), draws)
        return n_new


def inject_noise(gaussians, step_scale, seed, iteration, normals=None):
    """_xyz += R diag(s^2) R^T (z g step_scale) in place, z the normals of (seed, iteration) -- or `normals` (P, 3),
    for a caller who wants another generator's."""
    with torch.no_grad():
        if gaussians._xyz.shape[0] == 0:
            return
        if _fused(gaussians):
            from . import _C
            _C.mcmc_noise(gaussians._xyz.data, gaussians._scaling.data, gaussians._rotation.data, gaussians._opacity.data,
                          float(step_scale), _seed(seed), int(iteration),
                          None if normals is None else normals.detach().contiguous())
            return
        if normals is None:
            normals = torch.from_numpy(normals_numpy(gaussians._xyz.shape[0], _seed(seed), iteration)).to(
                gaussians._xyz.device)
        gaussians._xyz.data += noise_delta_torch(gaussians._scaling, gaussians._rotation, gaussians._opacity, step_scale,
                                                 normals)


def regulariser_and_grad(gaussians, w_opacity, w_scale):
    """The value w_opacity mean(get_opacity) + w_scale mean(get_scaling) (a detached 0-dim tensor), its gradient ADDED
    to _opacity.grad and _scaling.grad (made as zeros where a parameter has none yet): the term's share of the step,
    applied after the backward and before the optimizer as add_regulation_grad's is."""
    with torch.no_grad():
        o, s = gaussians._opacity, gaussians._scaling
        for p in (o, s):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        P = o.shape[0]
        if P == 0:
            return torch.zeros((), device=o.device)
        if _fused(gaussians):
            from . import _C
            return _C.mcmc_reg_grad(o.data, s.data, float(w_opacity), float(w_scale), o.grad, s.grad)
        sig, ex = torch.sigmoid(o.data), torch.exp(s.data)
        o.grad += (float(w_opacity) / P) * (sig * (1 - sig))
        s.grad += (float(w_scale) / (3 * P)) * ex
        return float(w_opacity) * sig.mean() + float(w_scale) * ex.mean()
