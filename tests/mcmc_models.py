"""Small CPU models for the MCMC densification tests (tests/test_mcmc_boundary.py, tests/test_mcmc_gpu.py): a
GaussianModel with chosen dead rows and non-zero moments and statistics, and a snapshot of everything a row plan
touches."""
import numpy as np
import torch

PARAM_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
STAT_ATTRS = ("xyz_gradient_accum", "denom", "max_radii2D", "_deformation_accum")


def make_model(P=40, seed=0, dead=(3, 4, 17, 30, 39), stepped=True):
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    hyper, opt = config.dnerf()
    torch.manual_seed(seed)
    g = GaussianModel(3, hyper, fused=False)
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    g._xyz = torch.nn.Parameter(f32(rng.normal(size=(P, 3))))
    g._features_dc = torch.nn.Parameter(f32(rng.normal(size=(P, 1, 3))))
    g._features_rest = torch.nn.Parameter(f32(rng.normal(size=(P, 15, 3))))
    g._scaling = torch.nn.Parameter(f32(rng.normal(-3, 0.5, size=(P, 3))))
    g._rotation = torch.nn.Parameter(f32(rng.normal(size=(P, 4))))
    raw = rng.normal(size=(P, 1))
    raw[list(dead)] = -8.0  # sigmoid(-8) = 3.4e-4: dead
    g._opacity = torch.nn.Parameter(f32(raw))
    g.max_radii2D = torch.zeros(P)
    g._deformation_table = torch.tensor(rng.random(P) > 0.3)
    g.spatial_lr_scale = 1.0
    g.training_setup(opt)
    if stepped:  # one optimizer step with random gradients: every moment and statistic is non-zero
        for a in PARAM_ATTRS:
            p = getattr(g, a)
            p.grad = f32(rng.normal(size=tuple(p.shape)))
        g.optimizer.step()
        g.optimizer.zero_grad(set_to_none=True)
        g.xyz_gradient_accum += 1.5
        g.denom += 2.0
        g.max_radii2D += 7.0
        g._deformation_accum += 0.25
    return g, hyper, opt


def moments(g):
    from gs4d_train import mcmc
    return mcmc._moments(g)


def snapshot(g):
    s = {a: getattr(g, a).detach().clone() for a in PARAM_ATTRS}
    s["table"] = g._deformation_table.clone()
    s["moments"] = [m.clone() for m in moments(g)]
    s["stats"] = [getattr(g, n).clone() for n in STAT_ATTRS]
    return s
