"""Device time of the train step's smaller HIP passes at its shapes (diagnostic, GPU): the first deformation
layer's backward (P = 100k, 32 -> 128), the deformation tail both ways, HIP events over R calls, and the image
losses (L1; SSIM and the fused L1 + D-SSIM beside torch's losses.ssim) with the spread over 9 rounds of R calls.
For A/B of libgs4d variants (LD_LIBRARY_PATH=4dgaussians-fast-train_amd/build/variant_<name>).
Usage: small_kernels_time.py [--ssim-only]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
from gs4d_train import _C  # noqa: E402


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    P, Fin, Fout = 100_000, 32, 128
    torch.manual_seed(0)
    x = torch.randn(P, Fin, device="cuda")
    w = torch.randn(Fout, Fin, device="cuda") / Fin ** 0.5
    b = torch.randn(Fout, device="cuda") * 0.1
    h = _C.feature_relu_forward(x, w, b)[0]
    g = torch.randn(P, Fout, device="cuda")
    rows = [("feature_relu_forward", lambda: _C.feature_relu_forward(x, w, b)),
            ("feature_relu_forward (+hb)", lambda: _C.feature_relu_forward(x, w, b, with_hb=True)),
            ("feature_relu_backward", lambda: _C.feature_relu_backward(g, h, x, w))]
    # the HexPlane regulariser's gradient (+ value) at DyNeRF's planes (F = 16, [64, 64, 64, 150] x multires [1, 2])
    from gs4d_train.kernels import hexplane_regulation_accumulate_grad
    grids = []
    for reso in ([64, 64, 64, 150], [128, 128, 128, 150]):
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        grids.append([torch.rand(1, 16, reso[c1], reso[c0], device="cuda").requires_grad_(True) for c0, c1 in pairs])
    for lvl in grids:
        for q in lvl:
            q.grad = torch.zeros_like(q)
    rows.append(("reg accumulate + value", lambda: hexplane_regulation_accumulate_grad(grids, 1.0, 1e-4, 2e-4, 1.0, True)))
    rows.append(("reg accumulate", lambda: hexplane_regulation_accumulate_grad(grids, 1.0, 1e-4, 2e-4, 1.0, False)))
    # the L1 value + gradient at the bench image (3 x 1014 x 1352)
    img, gt = torch.rand(3, 1014, 1352, device="cuda"), torch.rand(3, 1014, 1352, device="cuda")
    rows.append(("l1_loss_grad", lambda: _C.l1_loss_grad(img, gt, 1.0)))
    for name, fn in ([] if "--ssim-only" in sys.argv else rows):
        print(f"{name:28s} {timed(fn):8.1f} us", flush=True)
    # SSIM forward + backward and the fused L1 + D-SSIM (two launches each) beside losses.ssim forward + backward
    # (torch: grouped conv2d + element-wise + autograd) on the same tensors: median [min, max] of 9 rounds
    from gs4d_train.kernels import l1_dssim_loss_and_grad, ssim
    from gs4d_train.losses import ssim as ssim_torch

    def fwd_bwd(f, x, y):
        xa = x.detach().requires_grad_(True)
        f(xa, y).backward()

    for shape in ((1, 3, 1014, 1352), (1, 3, 800, 800)):
        x, y = torch.rand(shape, device="cuda"), torch.rand(shape, device="cuda")
        n = x.numel()
        for name, fn, nbytes in ((f"ssim fwd+bwd {shape[2]}x{shape[3]}", lambda: fwd_bwd(ssim, x, y), 44 * n),
                                 (f"ssim value only {shape[2]}x{shape[3]}", lambda: ssim(x, y), 8 * n),
                                 (f"l1_dssim_loss_grad {shape[2]}x{shape[3]}", lambda: l1_dssim_loss_and_grad(x, y, 0.2), 44 * n),
                                 (f"losses.ssim fwd+bwd {shape[2]}x{shape[3]}", lambda: fwd_bwd(ssim_torch, x, y), None)):
            ts = sorted(timed(fn) for _ in range(9))
            rate = f"  {nbytes / ts[4] / 1e6:6.2f} TB/s of its {nbytes / 1e6:.0f} MB" if nbytes else ""
            print(f"{name:32s} {ts[4]:8.1f} us [{ts[0]:.1f}, {ts[-1]:.1f}]{rate}", flush=True)


if __name__ == "__main__":
    main()
