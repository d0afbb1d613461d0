"""GPU tests of the blend backward on short tile lists: one- and two-tile images (16x16, 17x9, 32x16) whose lists hold
exactly 1, 2, 3, 63, 64, 65 or 129 splats (tests/short_run_scenes.py) -- an odd last pair, a full batch, a batch
boundary -- through the colour, depth, aux and absgrad backward entries.

Colour: forward and backward against the CPU oracle with the bars of tests/test_gpu_parity.py (its _check).  All four
entries: every element against the fp64 restatement with the bar of tests/test_rule_branches_gpu.py,
|gpu - ref| <= GRAD_RTOL |ref| + F max|ref|, F = max(GRAD_FLOOR, 2 F_oracle) with F_oracle the floor the fp32 oracle's
colour backward needs against fp64 on the same scene.  tests/test_backward_short_runs_boundary.py asserts on the CPU
that no scene carries a flip flag; the conditions are asserted again here before anything is compared.
"""
import numpy as np
import pytest
import torch

import short_run_scenes as SR
from gpu_helpers import c_forward, o_backward, to_dev
from oracle import parity as PAR
from test_depth_grad_gpu import needed_floor
from test_gpu_parity import _check
from test_rule_branches_gpu import ENTRIES, NAMES8, _pairs, _ratio

pytestmark = pytest.mark.gpu


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def backward(entry, s, d, fwd, grads):
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = fwd
    imgs = [torch.tensor(np.ascontiguousarray(x), device="cuda:0") for x in grads]
    return getattr(_C(), entry)(
        d["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], float(s["scale_modifier"]), e, d["viewmatrix"],
        d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), *imgs, d["shs"], int(s["sh_degree"]), d["campos"],
        gb, nr, bb, ib, False)


@pytest.mark.parametrize("case", SR.CASES, ids=SR.case_id)
def test_colour_path_matches_the_oracle(oracle, case):
    SR.preconditions(oracle, case)
    report = []
    _check(_C(), oracle, SR.scene(case)["s"], torch.device("cuda:0"), report=report)
    assert report[0]["L"] == case[2] * ((case[0] + 15) // 16) * ((case[1] + 15) // 16)
    assert report[0]["flagged_pix_frac"] == 0 and report[0]["flagged_gauss_frac"] == 0


@pytest.mark.parametrize("case", SR.CASES, ids=SR.case_id)
def test_backward_entries_match_fp64(oracle, case):
    SR.preconditions(oracle, case)
    sc, r = SR.scene(case), SR.reference(oracle, case)
    s = sc["s"]
    g_c, g_d, g_a = SR.upstream(oracle, case, "color")
    f_oracle = needed_floor(_pairs(o_backward(oracle, s, r["state"], r["radii"], g_c),
                                   SR.autograd_grads(oracle, case, g_c, g_d, g_a), r["radii"]))
    F = max(PAR.GRAD_FLOOR, 2.0 * f_oracle)
    d = to_dev(s, torch.device("cuda:0"))
    fwd = c_forward(_C(), s, d)
    radii = fwd[3].cpu().numpy()
    assert fwd[0] == r["nr"] and np.array_equal(radii, r["radii"])
    failures = []
    for entry, (n_img, kind) in ENTRIES.items():
        ups = SR.upstream(oracle, case, kind)
        got = backward(entry, s, d, fwd, ups[:n_img])
        pairs = _pairs(got[:8], SR.autograd_grads(oracle, case, *ups), radii)
        assert [n for n, _, _ in pairs][:5] == NAMES8[:5]
        worst = {n: _ratio(a, b, F) for n, a, b in pairs}
        assert got[2].abs().max() > 0 and got[3].abs().max() > 0
        if entry.endswith("absgrad"):
            assert len(got) == 9
            absg = got[8].cpu().numpy().astype(np.float64)
            assert np.isfinite(absg).all() and not np.any(absg[:, 2]) and np.all(absg >= 0)
            want = SR.absgrad(oracle, case, *ups)
            assert want.max() > 0
            worst["absgrad"] = _ratio(absg[:, :2], want, F)
        else:
            assert len(got) == 8
        print(f"[short-runs] {SR.case_id(case)} {entry.replace('rasterize_gaussians_', '')}: F_oracle = "
              f"{f_oracle:.3e}, F = {F:.3e}; worst ratios " + " ".join(f"{n}={v:.3f}" for n, v in worst.items()),
              flush=True)
        failures += [f"{entry} {n}: an element off by {v:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"
                     for n, v in worst.items() if not v <= 1.0]
    assert not failures, "; ".join(failures)
