"""Cost of the MCMC strategy's per-step work (diagnostic, GPU).

Reports, the rows alternated inside every round of this one process after a warm-up of each, HIP events around CALLS
calls, microseconds per call, median [min .. max] over ROUNDS rounds, at P = 100,000 Gaussians:
  the noise: the fused launch (mcmc.inject_noise on a fused model) against its torch formulation (build_rotation, two
  bmm, the gate, randn for the normals -- what the step would run without the kernel);
  the regulariser: the fused value + gradient against the torch formulation through autograd (both add to existing
  .grad buffers);
  the fine-stage train step (one 320 x 240 view) with densify_strategy "mcmc" against "default", at equal P, at
  iterations where neither strategy changes the rows, both models stepped alternately; the mcmc model runs with zero
  regulariser weights and a zero noise scale, so that every launch of the strategy runs and both models stay the same
  scene (with the default weights the regulariser reaches every Gaussian's Adam step and the scenes drift apart
  within tens of steps: the rows would compare two renders, not two strategies);
  one refinement event: relocate + grow on a model with 5 % dead rows.  The rows are put back before every call (a
  surgery.apply that drops the grown rows and an indexed opacity write), which the row includes; a second row runs one
  more restore, so the difference of the two is the restore's cost and the event alone is the first row minus it.
No time bar is set: the rows are reported.  --small: 4,000 points (a rehearsal, not a measurement)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
from gs4d_train import config, mcmc  # noqa: E402
from gs4d_train.gaussians import GaussianModel  # noqa: E402
from gs4d_train.synthetic import make_point_cloud, make_training_views  # noqa: E402
from gs4d_train.train import train_step  # noqa: E402

CALLS, ROUNDS = 5, 9


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(rows):
    for fn in rows.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in rows}
    for _ in range(ROUNDS):
        for k, fn in rows.items():
            res[k].append(timed_us(fn, CALLS))
    for k, v in res.items():
        print(f"  {k:52s} {statistics.median(v):10.1f} us  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)
    return res


def model(P, strategy):
    hyper, opt = config.dynerf()
    opt.densify_strategy = strategy
    opt.densify_from_iter = 10 ** 9  # no strategy changes the rows: the steps compare at equal P
    opt.opacity_reset_interval = 10 ** 9
    pts, cols = make_point_cloud(P, seed=5)
    torch.manual_seed(7)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = True
    g._deformation.deformation_net.fused_heads = True
    g.training_setup(opt)
    g.active_sh_degree = 3
    return g, hyper, opt


def main():
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "mcmc_time.py measures on the GPU"
    P = 4_000 if small else 100_000
    print(f"mcmc_time: P = {P}; {CALLS} calls x {ROUNDS} alternating rounds; median [min .. max]")
    g, hyper, opt = model(P, "mcmc")
    dev = g._xyz.device

    def torch_noise():
        z = torch.randn(P, 3, device=dev)
        g._xyz.data += mcmc.noise_delta_torch(g._scaling, g._rotation, g._opacity, 1e-3, z)

    def torch_reg():
        value = 0.01 * g.get_opacity.mean() + 0.01 * g.get_scaling.mean()
        value.backward()
        return value

    def fused_reg():
        return mcmc.regulariser_and_grad(g, 0.01, 0.01)

    print("the per-step pieces")
    alternate({"noise: fused launch": lambda: mcmc.inject_noise(g, 1e-3, 0, 1),
               "noise: torch formulation (randn, bmm, gate)": torch_noise,
               "regulariser: fused value + gradient": fused_reg,
               "regulariser: torch formulation + autograd": torch_reg})
    g.optimizer.zero_grad(set_to_none=True)

    views = make_training_views(2, 320, 240, seed=6)
    bg = torch.ones(3, device=dev)
    gd, hyper_d, opt_d = model(P, "default")
    # a fresh model with the default one's rows; zero weights and a zero noise scale run every launch of the strategy
    # and add zeros, so both models keep the same parameters step after step: the two rows render the same scene
    g, hyper, opt = model(P, "mcmc")
    opt.mcmc_opacity_reg = opt.mcmc_scale_reg = opt.mcmc_noise_lr = 0.0
    it = [3001]

    def step(gm, hy, op):
        def run():
            it[0] += 1
            train_step(gm, views[it[0] % 2:it[0] % 2 + 1], op, hy, it[0], bg)
        return run
    print("the fine-stage train step, one 320 x 240 view")
    alternate({"train step, densify_strategy = \"default\"": step(gd, hyper_d, opt_d),
               "train step, densify_strategy = \"mcmc\"": step(g, hyper, opt)})
    print("the same, the other order inside a round")
    alternate({"train step, densify_strategy = \"mcmc\"": step(g, hyper, opt),
               "train step, densify_strategy = \"default\"": step(gd, hyper_d, opt_d)})

    ge, _, _ = model(P, "mcmc")
    state = None

    def restore():
        nonlocal state
        if state is None:  # moments exist from here on
            for p in (ge._xyz, ge._features_dc, ge._features_rest, ge._opacity, ge._scaling, ge._rotation):
                p.grad = torch.zeros_like(p)
            ge.optimizer.step()
            ge.optimizer.zero_grad(set_to_none=True)
            state = True
        from gs4d_train import surgery
        if ge._xyz.shape[0] != P:
            surgery.apply(ge, surgery.RowPlan(keep=torch.arange(P, device=dev)))
        with torch.no_grad():
            ge._opacity[::20] = -8.0

    def event():
        restore()
        mcmc.relocate(ge, 0, 100, 0.005)
        mcmc.grow(ge, 0, 100, 10 ** 9, 0.005)

    def restore_alone():
        event()      # untimed work cannot be kept out of a row: the restore is timed on rows an event has grown,
        restore()    # so this row is the first one plus one more restore, and the difference is the restore's cost
    print("one refinement event (5 % dead rows relocated, 5 % growth): the rows are put back before every event, so the")
    print("event alone is the first row minus (second - first)")
    alternate({"restore + relocate + grow": event, "restore + relocate + grow + restore": restore_alone})


if __name__ == "__main__":
    main()
