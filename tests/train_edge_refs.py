"""Float64 restatements of the train-step tail kernels' documented formulas (include/gs4d_train.h), with the
planted edge-case inputs the edge tests share (test infrastructure, next to torch_restatement.py).

Every helper takes the kernels' fp32 inputs, casts them to double and evaluates the header's formula once.  Beside
each value it returns the element's MAGNITUDE (the sum of the absolute values of the terms that form it) and the
count c of fp32 roundings on the element's path, as a `Ref`.  An fp32 implementation may differ from the value by

    bar = c * 2^-24 * magnitude + floor

2^-24 is fp32's unit roundoff: one correctly rounded operation contributes 1 to c; an expf, sqrtf or divide is
allowed 2 ulp = 4 units (an ulp is 2^-23).  floor is 2^-126, the smallest normal fp32, times the factors that
multiply the element afterwards: below it fp32 has no relative precision (and an intermediate such as exp(100)
leaves the format), so a result in that range is only asked to be that small.  c == 0 marks a result the header
promises exactly (copies, zeros, counts).  No bar depends on what a kernel produced.  Device-agnostic: the
helpers run where their inputs live, and test_harness_cpu checks them against torch's own fp32 graphs on the CPU.
"""
import collections

import numpy as np
import torch

U = 2.0 ** -24                              # fp32 unit roundoff
TINY = 2.0 ** -126                          # smallest normal fp32
ULP2 = 4                                    # "2 ulp" in units of 2^-24
EPS_NORMALIZE = float(np.float32(1e-12))    # F.normalize's eps as the kernels hold it (1e-12f)


class Ref(collections.namedtuple("Ref", "val mag c floor")):
    """val, mag: float64 tensors; c: rounding count (a number or a tensor); floor: absolute floor (same)."""

    @property
    def bar(self):
        return self.c * U * self.mag + self.floor


def _d(t):
    return None if t is None else t.detach().double()


def _exact(val):
    return Ref(val, val.abs(), 0, 0.0)


def worst(got, ref):
    """Largest error of `got` as a fraction of its bar (0 where both the error and the bar are 0, inf for a
    non-finite result or an error where the bar is 0)."""
    err = (got.detach().double() - ref.val).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    bar = torch.as_tensor(ref.bar, dtype=torch.float64, device=err.device).expand_as(err)
    frac = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(frac.max()) if frac.numel() else 0.0


# ---- deformation tail (gs4d_deform_tail_forward / _backward) ------------------------------------------------
def deform_tail_ref(base, deltas, ups=None):
    """base = (xyz, s, r, o, f_dc, f_rest), deltas = (dx, ds, dr, do, dshs (P, 3K)) with None for a head that is
    off, ups = the five outputs' upstream gradients (None: that output is unused).  Returns (outputs, grads):
    dicts of Ref.  The gradient of each delta is the gradient of its base; d_shs is the flat gradient of dshs."""
    xyz, s, r, o, f_dc, f_rest = (_d(t) for t in base)
    dx, ds, dr, do, dshs = (_d(t) for t in deltas)
    P = xyz.shape[0]
    z = lambda t: torch.zeros_like(t)
    has = lambda t: 0 if t is None else 1
    add = lambda a, b: a if b is None else a + b
    mag_add = lambda a, b: a.abs() if b is None else a.abs() + b.abs()
    out = {}
    out["means"] = Ref(add(xyz, dx), mag_add(xyz, dx), has(dx), 0.0)            # one add
    xs = add(s, ds)
    # expf: 2 ulp; the argument's rounding (one add) moves exp by |s + ds| * 2^-24 relative
    c_scales = ULP2 + has(ds) * xs.abs()
    out["scales"] = Ref(torch.exp(xs), torch.exp(xs), c_scales, TINY)
    q = add(r, dr)
    n = q.pow(2).sum(-1, keepdim=True).sqrt()
    nrm = n.clamp_min(EPS_NORMALIZE)
    # q_c: one add; |q|: that add again, 4 roundings in the sum of squares (4 products' and 3 adds' share of
    # sqrt(1 + d) = 1 + d / 2), sqrtf 2 ulp; the divide 2 ulp
    out["rot"] = Ref(q / nrm, (q / nrm).abs(), 2 * has(dr) + 4 + ULP2 + ULP2, TINY)
    xo = add(o, do)
    y = torch.sigmoid(xo)
    # e = expf(-x): 2 ulp + |x| * 2^-24 from the add; 1 + e: one add (e's error enters with weight e / (1 + e)
    # <= 1); the divide 2 ulp
    c_opac = ULP2 + has(do) * xo.abs() + 1 + ULP2
    out["opac"] = Ref(y, y, c_opac, TINY)
    sh = torch.cat((f_dc, f_rest), dim=1)
    d3 = None if dshs is None else dshs.reshape(sh.shape)
    out["shs"] = Ref(add(sh, d3), mag_add(sh, d3), has(dshs), 0.0)
    if ups is None:
        return out, None
    g_means, g_scales, g_rot, g_opac, g_shs = (_d(t) for t in ups)
    gr = {}
    gr["d_xyz"] = _exact(z(xyz) if g_means is None else g_means)
    if g_scales is None:
        gr["d_s"] = _exact(z(s))
    else:  # g * scales: scales' own error, one product
        v = g_scales * torch.exp(xs)
        gr["d_s"] = Ref(v, v.abs(), c_scales + 1, TINY * (1 + g_scales.abs()))
    if g_rot is None:
        gr["d_r"] = _exact(z(r))
    else:
        above = n > EPS_NORMALIZE
        t0 = g_rot / nrm
        qg = q * g_rot
        n3 = torch.where(above, n, torch.ones_like(n)) ** 3
        tj = torch.where(above, q.abs() * qg.abs().sum(-1, keepdim=True) / n3, z(q))
        v = t0 - torch.where(above, q * qg.sum(-1, keepdim=True) / n3, z(q))
        # with e_n = 7 (|q|: the add 1, the sum of squares 4 / 2, sqrtf 4):
        #   g / |q|: e_n + divide 4 = 11;
        #   q_c (q . g) / |q|^3 as (-(q . g) / (|q| |q|)) * (q_c / |q|): the dot product 5 (q_j's add, a product,
        #   3 adds), |q| |q| 2 e_n + 1 = 15, its divide 4, q_c / |q| 1 + e_n + 4 = 12, the product 1: 37;
        #   the final add 1 on the whole: c = 38.  At or below eps the result is g / eps: the divide alone, 4.
        gr["d_r"] = Ref(v, t0.abs() + tj, (above.double() * (38 - ULP2) + ULP2).expand_as(v), TINY)
    if g_opac is None:
        gr["d_o"] = _exact(z(o))
    else:  # (g (1 - y)) y = g y - g y y: y's own error (d/dy = g (1 - 2 y), |1 - 2 y| <= 1 + y), 1 - y, two products
        v = g_opac * y * (1 - y)
        gr["d_o"] = Ref(v, g_opac.abs() * y * (1 + y), c_opac + 3, TINY * (1 + g_opac.abs()))
    gs3 = z(sh) if g_shs is None else g_shs.reshape(sh.shape)
    gr["d_fdc"] = _exact(gs3[:, :1])
    gr["d_frest"] = _exact(gs3[:, 1:])
    gr["d_shs"] = _exact(gs3.reshape(P, -1))
    return out, gr


# planted rotation rows: r + dr (split evenly between r and dr when the head is on, so the sum is exact)
_ROT_ROWS = [
    None,                                   # r + dr == 0 exactly (dr = -r)
    (1.5e-13, -1.5e-13, 1.5e-13, 1.5e-13),  # norm 3e-13, below eps
    (1e-25, -1e-25, 1e-25, 1e-25),          # squares underflow in fp32
    (1e-12, 1e-12, -1e-12, 1e-12),          # norm 2e-12, just above eps
    (5e14, -5e14, 5e14, -5e14),             # norm 1e15
]
_S_VALS = (-80.0, 0.0, 80.0)
_O_VALS = (-100.0, -20.0, 0.0, 20.0, 100.0)
HEADS = {"all": (1, 1, 1, 1, 1), "none": (0, 0, 0, 0, 0), "mixed": (1, 0, 1, 0, 1)}


def deform_inputs(P, K, heads, device="cpu", seed=0):
    """(base, deltas, ups) for deform_tail at P rows, K SH coefficients; heads: a key of HEADS.  randn rows with the
    planted ones first (as many as fit; at P = 1 the zero quaternion, s + ds = (-80, 0, 80), o + do = 100) and a
    second zero quaternion in the last row.  planted_rows(P) lists the rows that hold one."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    on = HEADS[heads]
    base = [rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 1), rn(P, 1, 3), rn(P, K - 1, 3)]
    deltas = [rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 1), rn(P, 3 * K)]
    ups = [rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 1), rn(P, K, 3)]

    def plant(i, row, val):
        val = torch.tensor(val, dtype=torch.float32)
        if on[i]:
            base[i][row], deltas[i][row] = val / 2, val / 2
        else:
            base[i][row] = val
    for k, row in enumerate(_ROT_ROWS[:P]):
        if row is None:
            deltas[2][k] = -base[2][k]
            if not on[2]:
                base[2][k] = 0.0
        else:
            plant(2, k, row)
    if P > 1:
        deltas[2][P - 1] = -base[2][P - 1]
        if not on[2]:
            base[2][P - 1] = 0.0
    if P == 1:
        plant(1, 0, _S_VALS)
        plant(3, 0, (100.0,))
    else:
        for k, v in enumerate(_S_VALS[:P]):
            plant(1, k, (v, v, v))
        for k, v in enumerate(_O_VALS[:P]):
            plant(3, k, (v,))
    deltas = [d if on[i] else None for i, d in enumerate(deltas)]
    mv = lambda t: None if t is None else t.to(device)
    return [mv(t) for t in base], [mv(t) for t in deltas], [mv(t) for t in ups]


def planted_rows(P):
    return sorted(set(range(min(P, 5))) | {P - 1}) if P else []


# ---- densification statistics (gs4d_densify_stats) ----------------------------------------------------------
def densify_stats_ref(vs_grad, visible, radii, grad_accum, denom, max_radii):
    """The three mask forms: (visible, radii), (None, radii): radii > 0, (visible, None): max_radii untouched.
    Returns (grad_accum Ref, denom, max_radii, mask); denom and max_radii are exact (float64 of fp32 values)."""
    mask = visible if visible is not None else radii > 0
    m2 = mask.reshape(-1, *([1] * (grad_accum.dim() - 1)))
    v = _d(vs_grad)
    nrm = (v[:, 0] ** 2 + v[:, 1] ** 2).sqrt().reshape(grad_accum.shape)
    acc = _d(grad_accum)
    # sqrtf 2 ulp, two products, the add under the root, the accumulating add
    ref = Ref(torch.where(m2, acc + nrm, acc), torch.where(m2, acc.abs() + nrm, acc.abs()),
              m2.double() * (ULP2 + 2 + 2), 0.0)
    den = torch.where(m2.reshape(denom.shape), _d(denom) + 1, _d(denom))
    mr = _d(max_radii)
    if radii is not None:
        mr = torch.where(mask.reshape(mr.shape), torch.maximum(mr, radii.double().reshape(mr.shape)), mr)
    return ref, den, mr, mask


def densify_inputs(P, device="cpu", seed=0):
    """viewspace_grad as the [:, :3] slice of a (P, 4) tensor (non-contiguous), a visibility mask, radii with
    zeros (some of them on visible rows), (P, 1) accumulators and (P,) max_radii."""
    g = torch.Generator().manual_seed(seed)
    vs4 = torch.randn(P, 4, generator=g)
    vis = torch.rand(P, generator=g) > 0.3
    radii = torch.randint(0, 40, (P,), generator=g, dtype=torch.int32)
    radii[::3] = 0
    if P:
        vis[0] = True  # visible with radius 0
    acc = torch.rand(P, 1, generator=g)
    den = torch.randint(0, 5, (P, 1), generator=g).float()
    mr = torch.rand(P, generator=g) * 30
    return tuple(t.to(device) for t in (vs4, vis, radii, acc, den, mr))


# ---- Adam (gs4d_adam_step) ----------------------------------------------------------------------------------
def adam_ref(p, g, m, v, beta1, beta2, eps, neg_step_size, bias_correction2_sqrt):
    """One step by the header's formula, the scalars as the caller's doubles.  Returns Refs (exp_avg, exp_avg_sq,
    param)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    m2 = m + omb1 * (g - m)
    # the scalar 1 - beta1 to fp32, g - m, the fma
    rm = Ref(m2, m.abs() + omb1 * (g.abs() + m.abs()), 3, 0.0)
    v2 = beta2 * v + omb2 * g * g
    # the scalars beta2 and 1 - beta2 to fp32, v * beta2, g * g, the fma; g * g may underflow: the floor
    rv = Ref(v2, v2, 5, TINY)
    root = v2.sqrt()
    den = root / bias_correction2_sqrt + eps
    p2 = p + neg_step_size * m2 / den
    mag = p.abs() + abs(neg_step_size) * rm.mag / den
    # exp_avg 3; the denominator 14 (exp_avg_sq's 5 halved by the root, sqrtf 4, the scalar and the divide 1 + 4,
    # eps to fp32 1, the add 1: 13.5); m / den: 4; the step size to fp32 1; the fma 1: c = 23.  The floor:
    # exp_avg_sq's own floor moves the root by sqrt(v + 2^-126) - sqrt(v), which vanishes for a normal v
    floor = abs(neg_step_size) * rm.mag / den * ((v2 + TINY).sqrt() - root) / (bias_correction2_sqrt * den)
    return rm, rv, Ref(p2, mag, 23, floor)


ADAM_SIZES = (1, 3, 4, 5, 130, 4095, 4096, 4097, 4099, 8194)
ADAM_LR = 1e-3
ADAM_HYPER = ((0.9, 0.999), 1e-15), ((0.8, 0.99), 1e-8)   # (betas, eps) of the two param groups


def adam_case(n, device="cpu", seed=0):
    """n parameters with sizes cycling through ADAM_SIZES, every other one stored 4 bytes past 16-byte alignment;
    parameter n // 2 and the last one have zero elements; parameter 4 (130 elements) is (10, 13) and takes its
    gradient as a transposed view; parameter 5's gradient is None at the second step."""
    g = torch.Generator().manual_seed(seed)
    params = []
    for i in range(n):
        size = 0 if i in (n // 2, n - 1) else ADAM_SIZES[i % len(ADAM_SIZES)]
        t = torch.randn(size, generator=g)
        if i == 4:
            params.append(t.reshape(10, 13).to(device))
        elif i % 2:
            store = torch.zeros(size + 1, device=device)
            store[1:] = t.to(device)
            params.append(store[1:])
        else:
            params.append(t.to(device))
    return params


def adam_grads(params, step, seed=0):
    """The gradients of step `step` (0-based): randn scaled by 1e-3, 1 or 1e3 (by parameter and step), with an exact
    0 at element 0, 1e-25 (its square underflows) at 1, +1e18 at 2 and -1e18 at 3 where the size allows."""
    g = torch.Generator().manual_seed(1000 * (step + 1) + seed)
    out = []
    for i, p in enumerate(params):
        if i == 5 and step == 1:
            out.append(None)
            continue
        n = p.numel()
        t = torch.randn(n, generator=g) * (1e-3, 1.0, 1e3)[(i + step) % 3]
        if n >= 3:
            t[0], t[1], t[2] = 0.0, 1e-25, 1e18
        if n >= 4:
            t[3] = -1e18
        if i == 4:
            out.append(t.reshape(13, 10).to(p.device).t())
        else:
            out.append(t.to(p.device).reshape(p.shape))
    return out


def adam_scalars(lr, beta1, beta2, step):
    """(neg_step_size, bias_correction2_sqrt) in double, as torch.optim.Adam forms them for 1-based `step`."""
    return -(lr / (1 - beta1 ** step)), (1 - beta2 ** step) ** 0.5


# ---- L1 loss (gs4d_l1_loss_forward / _grad / _backward) ------------------------------------------------------
L1_PER_THREAD = 8   # kL1PerThread: fp32 adds per thread before the sums continue in fp64
L1_SIZES = (33 * 2048 - 4, 1, 17 * 2048 + 1, 4, 2048, 2, 16 * 2048, 2049, 3, 5, 2047, 16 * 2048 + 4, 8)


def l1_ref(x, y, dloss):
    """(value Ref, gradient): the mean as an fp64 sum; the gradient sign * fl32(dloss * fl32(1 / n)), exact."""
    d = _d(x) - _d(y)
    n = d.numel()
    val = d.abs().sum() / n
    scale = np.float32(dloss) * (np.float32(1.0) / np.float32(n))
    grad = (torch.sign(d) * float(scale)).float()
    # x - y, eight fp32 adds per thread, then fp64, then one rounding to fp32 (and one to spare)
    return Ref(val, val, L1_PER_THREAD + 3, 0.0), grad


def l1_inputs(n, device="cpu", seed=0):
    """x, y in [0, 1) with, where n allows: x - y = +1e-40 (a denormal, sign +1) in the last element, -1e-40 in the
    one before, exact ties at 0 (n >= 4) and 5 (n >= 8)."""
    g = torch.Generator().manual_seed(seed + n)
    x, y = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if n >= 2:
        x[n - 1], y[n - 1] = 1e-40, 0.0
    if n >= 3:
        x[n - 2], y[n - 2] = 0.0, 1e-40
    if n >= 4:
        y[0] = x[0]
    if n >= 8:
        y[5] = x[5]
    return x.to(device), y.to(device)
