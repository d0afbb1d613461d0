"""The fused SSIM / D-SSIM kernels (csrc/ssim.hip) against the formulation they restate, losses.ssim
(utils/loss_utils.py:36-66), evaluated in float64 on the same fp32 inputs (its window: the fp32 outer product
cast up).

Bars come from the reference formulation, never from the kernel: for each input losses.ssim is also run in fp32
on the same device with autograd; with eg = max |grad32 - grad64| and em = max |map32 - map64|, the fused
gradient must lie within 4 eg of grad64 at every element and the fused value (and each per-image value) within
4 em of the fp64 value (the mean's error is bounded by the map's largest error; the scalar's own fp32 error
cancels at random and is no usable bar).  Why 4: a separable filter rounds in a different order from the
121-tap form; a plain separable fp32 formulation used at most 1.6 of eg on every input class at these shapes,
which leaves a factor of 2.5, while a defect (a wrong tap, a lost halo, a missing term) moves elements by O(1)
of the gradient's size.  Each test prints the largest fraction of its bar it used ([ssim-bars])."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import train_edge_refs as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5, 7),      # image smaller than the window
          (1, 1, 11, 11),    # image equal to the window
          (2, 3, 16, 16),    # two images, per-image means
          (1, 3, 32, 32),    # exactly one tile
          (1, 3, 33, 65),    # one past a tile both ways
          (1, 3, 37, 53),    # W % 4 != 0, odd sizes
          (1, 3, 64, 80),    # interior tiles whose halos lie wholly inside the image
          (3, 37, 53),       # unbatched input
          "sliced"]          # (1, 3, 37, 53) as a non-contiguous view
CLASSES = ["uniform", "noisy", "equal", "flat", "binary"]
BAR = 4.0


def _inputs(shape, cls):
    """(x, y) on the GPU, fp32; "sliced": non-contiguous views of larger tensors."""
    g = torch.Generator().manual_seed(1000 * CLASSES.index(cls) + SHAPES.index(shape))
    sliced = shape == "sliced"
    full = (1, 3, 39, 60) if sliced else shape
    x = torch.rand(full, generator=g)
    if cls == "uniform":
        y = torch.rand(full, generator=g)
    elif cls == "noisy":
        y = (x + 0.02 * torch.randn(full, generator=g)).clamp(0, 1)
    elif cls == "equal":
        y = x.clone()
    elif cls == "flat":
        x = torch.full(full, 0.7)
        y = 0.7 + 0.01 * torch.rand(full, generator=g)
    else:
        x = (x > 0.5).float()
        y = (torch.rand(full, generator=g) > 0.5).float()
    x, y = x.cuda(), y.cuda()
    if sliced:
        x, y = x[:, :, 1:38, 3:56], y[:, :, 1:38, 3:56]
        assert not x.is_contiguous() and x.shape == (1, 3, 37, 53)
    return x, y


def _ssim_map(img1, img2):
    """losses.ssim restated so that it returns the map: the window is the fp32 outer product, cast to the
    images' dtype."""
    from gs4d_train.losses import create_window
    channel = img1.size(-3)
    window = create_window(11, channel).to(device=img1.device, dtype=img1.dtype)
    conv = lambda t: F.conv2d(t, window, padding=5, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def _upstream(B):
    """the non-uniform upstream vector of the size_average=False cases"""
    return torch.tensor([0.37, -1.25, 0.5, 2.0][:B], device="cuda")


@functools.lru_cache(maxsize=None)
def _reference(shape, cls):
    """Computed once per input and shared, never modified: the fp64 map, value, per-image values and gradients
    (of the mean; of sum(upstream * per-image means)), and the reference formulation's own fp32 errors em, eg
    and eg_per_image."""
    from gs4d_train.losses import ssim as ssim_torch
    x, y = _inputs(shape, cls)
    batched = x.dim() == 4
    with torch.no_grad():
        map64 = _ssim_map(x.double(), y.double())
        em = float((_ssim_map(x, y).double() - map64).abs().max())
    ref = {"em": em, "value": map64.mean(), "per_image": map64.flatten(1).mean(1) if batched else None}
    assert abs(float(ssim_torch(x.double(), y.double())) - float(ref["value"])) <= 1e-14  # the restatement is the formulation
    grads = {}
    for dtype in (torch.float64, torch.float32):
        xa = x.to(dtype).clone().requires_grad_(True)
        ssim_torch(xa, y.to(dtype)).backward()
        grads[dtype] = [xa.grad.double()]
        if batched:
            xa = x.to(dtype).clone().requires_grad_(True)
            (ssim_torch(xa, y.to(dtype), size_average=False) * _upstream(x.shape[0]).to(dtype)).sum().backward()
            grads[dtype].append(xa.grad.double())
    ref["grad"] = grads[torch.float64][0]
    ref["eg"] = float((grads[torch.float32][0] - ref["grad"]).abs().max())
    if batched:
        ref["grad_per_image"] = grads[torch.float64][1]
        ref["eg_per_image"] = float((grads[torch.float32][1] - ref["grad_per_image"]).abs().max())
    return ref


def _frac(got, want, bar):
    """largest error as a fraction of the bar (0 where the error is 0, inf for a non-finite result or an error
    where the bar is 0)"""
    err = (got.detach().double() - want).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    e = float(err.max()) if err.numel() else 0.0
    return 0.0 if e == 0.0 else (e / bar if bar > 0 else float("inf"))


def _report(what, fracs):
    print(f"\n[ssim-bars] {what}: largest error / bar = " + ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_ssim_value_and_gradient(shape, cls):
    from gs4d_train.kernels import ssim
    x, y = _inputs(shape, cls)
    ref = _reference(shape, cls)
    xa = x.clone().requires_grad_(True) if x.is_contiguous() else x.detach().requires_grad_(True)
    value = ssim(xa, y)
    up = 0.37
    (grad,) = torch.autograd.grad(value * up, xa)
    assert value.shape == () and grad.shape == x.shape
    fracs = {"value": _frac(value, ref["value"], BAR * ref["em"]),
             "grad": _frac(grad, up * ref["grad"], BAR * up * ref["eg"])}
    if cls == "equal":
        assert float(value) == 1.0
    if x.dim() == 4:
        xb = x.detach().requires_grad_(True)
        per_image = ssim(xb, y, size_average=False)
        assert per_image.shape == (x.shape[0],)
        (gpi,) = torch.autograd.grad((per_image * _upstream(x.shape[0])).sum(), xb)
        fracs["per-image value"] = _frac(per_image, ref["per_image"], BAR * ref["em"])
        fracs["per-image grad"] = _frac(gpi, ref["grad_per_image"], BAR * ref["eg_per_image"])
        if cls == "equal":
            assert bool((per_image == 1.0).all())
    _report(f"ssim {shape} {cls}", fracs)
    assert max(fracs.values()) <= 1.0, fracs


@functools.lru_cache(maxsize=None)
def _reference_combined(shape, cls, lam, dloss):
    """The train step's image loss dloss * (L1 + lambda (1 - ssim)) in the reference's formulation: its fp64
    gradient and the formulation's own fp32 error eg, as _reference's."""
    from gs4d_train.losses import l1_loss_torch, ssim as ssim_torch
    x, y = _inputs(shape, cls)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        xa = x.to(dtype).clone().requires_grad_(True)
        yd = y.to(dtype)
        (dloss * (l1_loss_torch(xa, yd) + lam * (1.0 - ssim_torch(xa, yd)))).backward()
        grads[dtype] = xa.grad.double()
    return grads[torch.float64], float((grads[torch.float32] - grads[torch.float64]).abs().max())


@pytest.mark.parametrize("lam,dloss", [(0.2, 1.0), (0.2, 0.5)])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 3, 33, 65), (1, 3, 37, 53), (1, 3, 64, 80)],
                         ids=lambda s: "x".join(map(str, s)))
def test_l1_dssim_loss_and_grad(shape, cls, lam, dloss):
    """dloss * (L1 + lambda (1 - ssim)) in one call: the SSIM value within 4 em of the fp64 value, the complete
    gradient within 4 eg of the fp64 gradient (eg: the fp32 error of the reference's formulation of this loss),
    the L1 value within the L1 bar of train_edge_refs."""
    from gs4d_train.kernels import l1_dssim_loss_and_grad
    x, y = _inputs(shape, cls)
    ref = _reference(shape, cls)
    want, eg = _reference_combined(shape, cls, lam, dloss)
    l1, value, grad = l1_dssim_loss_and_grad(x, y, lam, dloss)
    l1_val, _ = R.l1_ref(x, y, dloss)
    fracs = {"ssim": _frac(value, ref["value"], BAR * ref["em"]), "grad": _frac(grad, want, BAR * eg),
             "l1": R.worst(l1, l1_val)}
    _report(f"l1_dssim {shape} {cls} lambda {lam} dloss {dloss}", fracs)
    assert max(fracs.values()) <= 1.0, fracs
    if cls == "equal":
        assert float(value) == 1.0 and float(l1) == 0.0


def test_ssim_repeatable_and_no_grad_path():
    """Two calls give the same bits; the no-grad path gives the value bits of the grad path and allocates no
    maps (its peak allocation stays below one map's size)."""
    from gs4d_train.kernels import ssim
    x, y = _inputs((1, 3, 64, 80), "noisy")
    outs = []
    for _ in range(2):
        xa = x.clone().requires_grad_(True)
        v = ssim(xa, y)
        (g,) = torch.autograd.grad(v, xa)
        outs.append((v, g))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x2, y2 = _inputs((2, 3, 16, 16), "uniform")
    with torch.no_grad():
        ssim(x, y)  # the kept scratch exists from here on
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        v = ssim(x.clone().requires_grad_(True), y)
        peak = torch.cuda.max_memory_allocated() - before
        pi = ssim(x2, y2, size_average=False)
    assert not v.requires_grad and torch.equal(v, outs[0][0])
    assert peak < 2 * 4 * x.numel(), peak  # the clone and the results; the maps alone are 3 * 4 * numel
    assert torch.equal(ssim(x, y), outs[0][0])  # no gradient required: the same path
    pi_grad = ssim(x2.clone().requires_grad_(True), y2, size_average=False).detach()
    assert torch.equal(pi, pi_grad), (pi.tolist(), pi_grad.tolist())


_CROSS_PROCESS = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
from gs4d_train.kernels import ssim, l1_dssim_loss_and_grad
g = torch.Generator().manual_seed(3)
x = torch.rand(2, 3, 70, 101, generator=g).cuda().requires_grad_(True)
y = (x.detach().cpu() + 0.05 * torch.randn(2, 3, 70, 101, generator=g)).clamp(0, 1).cuda()
v = ssim(x, y)
(gx,) = torch.autograd.grad(v, x)
out = [v, gx, ssim(x.detach(), y, size_average=False), *l1_dssim_loss_and_grad(x, y, 0.2, 0.5)]
torch.cuda.synchronize()
print(hashlib.sha256(b"".join(t.detach().cpu().numpy().tobytes() for t in out)).hexdigest())
"""


def test_ssim_bitwise_across_processes():
    """Values and gradients of two fresh processes are the same bytes."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4dgaussians-fast-train_amd")
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", _CROSS_PROCESS, pkg], capture_output=True, text=True, timeout=55)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1] and len(digests[0]) == 64, digests


def test_ssim_argument_errors():
    from gs4d_train.kernels import ssim
    x, y = _inputs((1, 3, 32, 32), "uniform")
    with pytest.raises(ValueError):
        ssim(x, y, window_size=7)
    with pytest.raises(RuntimeError):
        ssim(x, y[:, :, :16])
    with pytest.raises(RuntimeError):
        ssim(x.cpu(), y.cpu())
