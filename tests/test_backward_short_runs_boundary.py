"""CPU test of the short-run scenes (tests/short_run_scenes.py, no GPU calls): every tile's list has the chosen length
and no decision of any scene lies in a flip band or near a threshold, so tests/test_backward_short_runs_gpu.py leaves
no element out of its comparison; and the fp32 oracle's colour backward matches the fp64 restatement on them within
the 2e-4 of tests/test_oracle.py.  Computed from the oracle and the restatement, never from the code under test."""
import numpy as np
import pytest

import short_run_scenes as SR
from gpu_helpers import o_backward
from oracle import parity as PAR


@pytest.mark.parametrize("case", SR.CASES, ids=SR.case_id)
def test_scene_preconditions(oracle, case):
    SR.preconditions(oracle, case)


@pytest.mark.parametrize("case", SR.CASES, ids=SR.case_id)
def test_oracle_matches_fp64_on_short_runs(oracle, case):
    sc, r = SR.scene(case), SR.reference(oracle, case)
    g_c, g_d, g_a = SR.upstream(oracle, case, "color")
    want = SR.autograd_grads(oracle, case, g_c, g_d, g_a)
    got = o_backward(oracle, sc["s"], r["state"], r["radii"], g_c)
    for n, a, b in zip(PAR.GRAD_NAMES, got, want):
        if b is None:
            continue
        a = a[:, :2] if n == "dL_dmeans2D" else a
        scale = max(float(np.abs(b).max()), 1e-12)
        assert float(np.abs(a - b.reshape(a.shape)).max()) / scale < 2e-4, n
