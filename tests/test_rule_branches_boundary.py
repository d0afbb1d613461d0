"""CPU tests of the rule-bound branches' scenes (no GPU calls): on every scene of tests/rule_scenes.py the rule the
scene is for binds, every discrete decision keeps its distance from its threshold (so the GPU tests of
tests/test_rule_branches_gpu.py compare every element), and the fp32 oracle's forward and hand-derived backward
match the fp64 restatement of those rules (tests/torch_restatement.py) within the bars of tests/test_oracle.py.

All of it is computed from the restatement and the oracle, never from the code under test.
"""
import numpy as np
import pytest
import torch

import rule_scenes as RS
from gpu_helpers import o_backward, o_bounds
from oracle import parity as PAR

CLAMP_MARGIN = 1e-4   # | |t.x / t.z| - lim | / lim of every Gaussian in a list
# |power| per unit of the magnitude of its terms, for the pairs whose sign decides a contribution: about 400 times
# the largest GPU-oracle operand difference per unit magnitude that oracle/parity.py records (2.31e-7)
POWER_MARGIN = 1e-4
TERM_MARGIN = 4e-4    # |T (1 - alpha) / 1e-4 - 1| of every blended or terminating slot: ten times FLIP_BAND_T


def preconditions(O, sc, r, g_c):
    """Assert the conditions under which every element of the scene can be compared; `sc` rule_scenes.scene's dict,
    `r` rule_scenes.reference's, g_c the colour gradient the flip bounds are carried with."""
    name, s, ref, ex = sc["name"], sc["s"], r["ref"], r["export"]
    b = o_bounds(O, s, r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    assert int((np.asarray(b["gflag"]) != 0).sum()) == 0 and int((np.asarray(b["pflag"]) != 0).sum()) == 0
    assert ref["near_threshold"] == 0
    assert np.array_equal(ref["n_contrib"], ex["n_contrib"])
    lens = (ex["ranges"][:, 1].astype(np.int64) - ex["ranges"][:, 0]).reshape(-1)
    vis = r["radii"] > 0
    if name.startswith("clamp"):
        assert int((ref["clamped"] & vis).sum()) >= 15, int((ref["clamped"] & vis).sum())
        assert ref["clamp_margin"] >= CLAMP_MARGIN, ref["clamp_margin"]
        fx, fy = s["W"] / (2 * s["tanfovx"]), s["H"] / (2 * s["tanfovy"])
        assert abs(fx - 60.6) < 0.05 and abs(fy - 71.4) < 0.05
        assert np.abs(s["viewmatrix"].reshape(4, 4)[:3, :3] - np.eye(3)).max() > 0.1
    else:
        assert ref["n_clamped"] == 0 and ref["clamp_margin"] >= CLAMP_MARGIN
    if name.startswith("clampmod"):
        assert s["scale_modifier"] == 0.7 and ref["scale_modifier"] == 0.7
    if name.startswith("indef"):
        nonpd = ref["nonpd"] & vis
        negated = np.arange(len(vis)) % sc["k"] == 0
        # the conics that are not positive definite belong to negated Gaussians, and each contributes somewhere
        assert nonpd.sum() >= 6 and not (nonpd & ~negated).any()
        assert ref["nonpd_contributes"][nonpd].all()
        assert ref["n_power_rejected"] >= 1000, ref["n_power_rejected"]
        assert ref["power_margin"] >= POWER_MARGIN, ref["power_margin"]
    else:
        assert not ref["nonpd"][vis].any() and ref["n_power_rejected"] == 0
    if name.startswith("indef_dense"):
        assert lens.min() >= 65 and lens.max() > 128 and (lens % 2 == 1).any()  # several batches, odd lengths
    if name.startswith("indef_small"):
        assert lens.max() < 64
    if name == "indef_dense_k29":
        # full 64-splat batches with and without a non-positive-definite conic within one tile's list
        def full_batches(tile):
            a, e = int(ex["ranges"][tile, 0]), int(ex["ranges"][tile, 1])
            return [bool(ref["nonpd"][ex["point_list"][i:i + 64]].any()) for i in range(a, e - 63, 64)]
        assert any(True in fb and False in fb for fb in map(full_batches, range(len(lens))))
    if name.startswith("term"):
        assert ref["n_terminated"] >= 100, ref["n_terminated"]
        assert ref["cap_blended"] >= 10, ref["cap_blended"]
        assert ref["term_margin"] >= TERM_MARGIN, ref["term_margin"]
        assert lens.max() > 64  # more than one batch
    else:
        assert ref["clamp099"] == 0 and ref["n_terminated"] == 0 and ref["min_T"] > 5e-3
        assert ref["term_margin"] >= TERM_MARGIN


@pytest.mark.parametrize("name", RS.NAMES)
def test_scene_preconditions(oracle, name):
    sc, r = RS.scene(name), RS.reference(oracle, name)
    ref = r["ref"]
    print(f"[rule-scenes] {name}: clamped {ref['n_clamped']} (margin {ref['clamp_margin']:.2e}), non-PD "
          f"{int(ref['nonpd'].sum())}, power > 0 pairs {ref['n_power_rejected']} (margin {ref['power_margin']:.2e}), "
          f"terminated pixels {ref['n_terminated']} (margin {ref['term_margin']:.2e}), cap binds on "
          f"{ref['cap_blended']} blended pairs, min T {ref['min_T']:.2e}", flush=True)
    preconditions(oracle, sc, r, RS.upstream(oracle, name, "color")[0])


@pytest.mark.parametrize("name", RS.NAMES)
def test_oracle_matches_the_restated_rules(oracle, name):
    """tests/test_oracle.py::test_oracle_backward_matches_autograd on the rule scenes, with its bars: colour 2e-6,
    depth 2e-5, final_T 2e-6, every gradient tensor within 2e-4 of its maximum; dL_dmeans3D also over the clamped
    rows alone (a maximum over all rows would hide an error there); culled rows exactly zero."""
    sc, r = RS.scene(name), RS.reference(oracle, name)
    s, ref = sc["s"], r["ref"]
    np.testing.assert_allclose(r["color"], ref["color"].detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(r["depth"], ref["depth"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(r["export"]["final_T"], ref["Tfinal"].detach().numpy(), atol=2e-6)
    g_c, g_d, g_a = RS.upstream(oracle, name, "color")
    want = RS.autograd_grads(oracle, name, g_c, g_d, g_a)
    got = o_backward(oracle, s, r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"],
                     use_sh=sc["use_sh"])
    vis = r["radii"] > 0
    worst = {}
    for n, a, b in zip(PAR.GRAD_NAMES, got, want):
        if b is None:
            continue
        a = a[:, :2] if n == "dL_dmeans2D" else a
        assert not np.any(a[~vis]), f"{n}: culled rows not zero"
        scale = max(float(np.abs(b[vis]).max()), 1e-12)
        worst[n] = float(np.abs(a[vis] - b[vis].reshape(a[vis].shape)).max()) / scale
    rows = ref["clamped"] & vis
    if name.startswith("clamp"):
        scale = float(np.abs(want[3][rows]).max())
        assert scale > 0
        worst["dL_dmeans3D[clamped]"] = float(np.abs(got[3][rows] - want[3][rows]).max()) / scale
    print(f"[rule-oracle] {name}: " + " ".join(f"{n}={v:.2e}" for n, v in worst.items()), flush=True)
    assert len(worst) >= 5
    for n, v in worst.items():
        assert v < 2e-4, f"{n}: rel err {v:.3e}"


def test_plain_clamp_autograd_is_not_the_reference(oracle):
    """The restated Q22 (which the oracle's backward matches on the clamped rows, above) differs from differentiating
    clamp(t.x / t.z) * t.z: there d(t.x_clamped)/d(t.z) = +-lim enters dL_dtz.  Same conic, and a gradient with
    respect to the clamped means that is off by more than 1e-2 of its maximum, fifty times the 2e-4 bar: the
    restatement cannot be 'simplified' to torch.clamp without the oracle test noticing."""
    import torch_restatement as TR
    name = "clamp1"
    sc, r = RS.scene(name), RS.reference(oracle, name)
    s = sc["s"]
    means = torch.tensor(s["means3D"], dtype=torch.float64, requires_grad=True)
    cov3 = TR.covariance(torch.tensor(s["scales"], dtype=torch.float64),
                         torch.tensor(s["rotations"], dtype=torch.float64))
    held = TR.projected_geometry(s, means, cov3)
    rows = torch.tensor(r["ref"]["clamped"] & (r["radii"] > 0))
    g_held = torch.autograd.grad(held["conic"][rows].sum(), means)[0][rows]
    # the same conic with the clamp differentiated through
    V = torch.tensor(s["viewmatrix"], dtype=torch.float64).reshape(4, 4)
    t = (torch.cat([means, torch.ones(len(means), 1, dtype=torch.float64)], 1) @ V)[:, :3]
    lim = torch.tensor([1.3 * s["tanfovx"], 1.3 * s["tanfovy"]], dtype=torch.float64)
    txy = torch.maximum(torch.minimum(t[:, :2] / t[:, 2:3], lim), -lim) * t[:, 2:3]
    fx, fy = s["W"] / (2 * s["tanfovx"]), s["H"] / (2 * s["tanfovy"])
    J = torch.zeros(len(means), 3, 3, dtype=torch.float64)
    J[:, 0, 0], J[:, 0, 2] = fx / t[:, 2], -fx * txy[:, 0] / t[:, 2] ** 2
    J[:, 1, 1], J[:, 1, 2] = fy / t[:, 2], -fy * txy[:, 1] / t[:, 2] ** 2
    Tm = J @ V[:3, :3].T
    c2 = Tm @ cov3 @ Tm.transpose(1, 2)
    a, b, c = c2[:, 0, 0] + 0.3, c2[:, 0, 1], c2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    assert torch.allclose(conic, held["conic"], rtol=1e-12, atol=0)  # the same value ...
    g_plain = torch.autograd.grad(conic[rows].sum(), means)[0][rows]
    assert float((g_plain - g_held).abs().max()) > 1e-2 * float(g_held.abs().max())  # ... another gradient
