"""The train step with D-SSIM on (opt.lambda_dssim != 0): the fused step takes the fused L1 + D-SSIM kernels
(gs4d_train.kernels.l1_dssim_loss_and_grad), matches the reference's torch formulation (fused=False), and
leaves the lambda_dssim == 0 step on the one-pass L1 it had."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(P, fused, hyper, opt, seed=7):
    from gs4d_train.gaussians import GaussianModel
    from gs4d_train.synthetic import make_point_cloud
    pts, cols = make_point_cloud(P, seed=5)
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=fused)
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = fused
    g._deformation.deformation_net.fused_heads = fused
    g.training_setup(opt)
    g.active_sh_degree = 3
    return g


def _config(lambda_dssim):
    from gs4d_train import config
    hyper, opt = config.dynerf()
    opt.iterations = 0  # the optimizer is held back: the parameter gradients themselves are compared
    opt.lambda_dssim = lambda_dssim
    return hyper, opt


@pytest.mark.parametrize("P,W,H", [(20000, 320, 240)])
def test_train_step_dssim_fused_matches_torch(P, W, H):
    """test_train_step_fused_matches_torch_tail's pattern with lambda_dssim = 0.2: one fine-stage step, fused
    against the torch formulation, the same bars for the same reason (fp32 summation order differs and the step
    amplifies ~1e-7 output differences through the L1 sign and the blend thresholds into isolated gradient
    elements): the loss within 1e-5 relative, every gradient within 1e-3 of its tensor's max and 1e-4 at the
    99.9th percentile."""
    from gs4d_train.synthetic import make_training_views
    from gs4d_train.train import train_step
    hyper, opt = _config(0.2)
    views = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")
    runs = []
    for fused in (False, True):
        g = _model(P, fused, hyper, opt)
        loss = float(train_step(g, views, opt, hyper, 3001, bg))
        grads = {n: p.grad.detach().clone() for n, p in g._deformation.named_parameters() if p.grad is not None}
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            grads[name] = getattr(g, name).grad.detach().clone()
        runs.append((loss, grads))
    (la, gra), (lb, grb) = runs
    print(f"\n[dssim-step] loss torch {la:.8f} fused {lb:.8f} relative difference {abs(lb - la) / abs(la):.2e}")
    assert abs(lb - la) <= 1e-5 * abs(la)
    assert gra.keys() == grb.keys()
    worst = (0.0, 0.0)
    for k in gra:
        a, b = gra[k], grb[k]
        scale = max(a.abs().max().item(), 1e-30)
        d = (a - b).abs().flatten() / scale
        p999 = d.kthvalue(max(1, int(0.999 * d.numel()))).values.item()
        worst = (max(worst[0], d.max().item()), max(worst[1], p999))
        assert d.max().item() < 1e-3, (k, d.max().item())
        assert p999 < 1e-4, k
    print(f"[dssim-step] largest gradient difference {worst[0]:.2e} of the max, 99.9th percentile {worst[1]:.2e}")


def test_fused_step_with_dssim_never_calls_torch_ssim(monkeypatch):
    """The fused step with lambda_dssim = 0.2 runs with losses.ssim out of reach; the fused=False step needs it."""
    import gs4d_train.losses
    from gs4d_train.synthetic import make_training_views
    from gs4d_train.train import train_step

    def refuse(*a, **k):
        raise AssertionError("losses.ssim called")

    monkeypatch.setattr(gs4d_train.losses, "ssim", refuse)
    hyper, opt = _config(0.2)
    views = make_training_views(1, 96, 64, seed=6)
    bg = torch.ones(3, device="cuda")
    loss = train_step(_model(3000, True, hyper, opt), views, opt, hyper, 3001, bg)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    with pytest.raises(AssertionError, match="losses.ssim called"):
        train_step(_model(3000, False, hyper, opt), views, opt, hyper, 3001, bg)


def test_step_without_dssim_keeps_the_one_pass_l1(monkeypatch):
    """lambda_dssim == 0: the fused step still takes kernels.l1_loss_and_grad (and only it), and two steps from
    the same seed give the same loss bits."""
    import gs4d_train.kernels as K
    from gs4d_train.synthetic import make_training_views
    from gs4d_train.train import train_step
    calls = []
    real = K.l1_loss_and_grad

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("the D-SSIM path ran with lambda_dssim == 0")

    monkeypatch.setattr(K, "l1_loss_and_grad", counted)
    monkeypatch.setattr(K, "l1_dssim_loss_and_grad", refuse)
    monkeypatch.setattr(K, "ssim", refuse)
    hyper, opt = _config(0.0)
    views = make_training_views(1, 96, 64, seed=6)
    bg = torch.ones(3, device="cuda")
    losses = [train_step(_model(3000, True, hyper, opt), views, opt, hyper, 3001, bg).clone() for _ in range(2)]
    assert len(calls) == 2
    assert torch.equal(losses[0], losses[1]) and bool(torch.isfinite(losses[0]))
