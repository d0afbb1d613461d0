"""One- and two-tile scenes whose tile lists have a chosen length, for the blend backward's pair walk (test
infrastructure; the shape of tests/rule_scenes.py, whose fp64 machinery it reuses).

Every splat is wide enough (3 sigma beyond the image's diagonal) to be listed in every tile, so each tile's list holds
all n Gaussians: n = 1, 2, 3 (an odd last pair next to the zero splat staged past the batch), 63, 64, 65 (a full
64-splat batch and the first splat past it) and 129 (two batch boundaries).  Images: 16x16 (one full tile), 17x9 (two
tiles, the second one pixel wide, both cut off below row 9) and 32x16 (two full tiles).  Opacities shrink with n so
that no pixel's transmittance comes near the 1e-4 termination, and the seeds are the first ones on which no decision
lies in a flip band (tests/test_backward_short_runs_boundary.py asserts both), so every element is compared.
"""
import math

import numpy as np

import rule_scenes as RS
from gs4d_train.synthetic import make_scene, make_upstream_grad

IMAGES = [(16, 16), (17, 9), (32, 16)]
LENGTHS = [1, 2, 3, 63, 64, 65, 129]
CASES = [(W, H, n) for (W, H) in IMAGES for n in LENGTHS]
# (W, H, n) -> seed: the first seed from 0 on which preconditions() holds; absent = 0.  The passed-over seeds of
# 17x9 leave one to three splats out of the one-pixel-wide second tile's list; 32x16 n = 129 seed 0 has a flip flag.
SEEDS = {(17, 9, 63): 1, (17, 9, 64): 1, (17, 9, 65): 1, (17, 9, 129): 3, (32, 16, 129): 1}


def case_id(case):
    return "%dx%d_n%d" % case


def build(W, H, n, seed):
    s = make_scene(n, W, H, seed=seed, sh_degree=3, spread=0.9, z_range=(2.0, 4.0), log_scale=math.log(1.2),
                   log_scale_sigma=0.2)
    u = np.random.default_rng(seed + 50).uniform(0.5, 1.0, (n, 1))
    s["opacities"] = (u * min(0.6, 4.0 / n)).astype(np.float32)
    return dict(name=case_id((W, H, n)), s=s, colors=None, cov3D=None, use_sh=True, mode="sh", k=0, seed=seed)


_CACHE, _REF, _FW = {}, {}, {}


def scene(case):
    if case not in _CACHE:
        _CACHE[case] = build(*case, SEEDS.get(case, 0))
    return _CACHE[case]


def reference(O, case):
    """rule_scenes.make_reference's dict: the oracle's forward and the fp64 autograd forward over its lists"""
    if case not in _REF:
        _REF[case] = RS.make_reference(O, scene(case))
    return _REF[case]


def upstream(O, case, kind):
    """rule_scenes.upstream's three gradient images ("color", "both" or "all") for the case"""
    assert kind in ("color", "both", "all")
    sc = scene(case)
    H, W, seed = sc["s"]["H"], sc["s"]["W"], sc["seed"]
    g_d = np.random.default_rng(1000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_a = np.random.default_rng(2000 + seed).normal(0, 1, (1, H, W)).astype(np.float32)
    g_c = (make_upstream_grad(reference(O, case)["color"], seed=seed + 1)[0] * (3 * W * H)).astype(np.float32)
    if kind == "color":
        g_d = np.zeros_like(g_d)
    if kind != "all":
        g_a = np.zeros_like(g_a)
    return g_c, g_d, g_a


def autograd_grads(O, case, g_c, g_d, g_a):
    return RS.grads_of(scene(case), reference(O, case)["ref"], g_c, g_d, g_a)


def absgrad(O, case, g_c, g_d, g_a):
    import absgrad_refs as AR
    if case not in _FW:
        s, ex = scene(case)["s"], reference(O, case)["export"]
        _FW[case] = AR.per_pixel_forward(s, ex["point_list"], ex["ranges"], s["sh_degree"], colors=None, cov3D=None)
    want = autograd_grads(O, case, g_c, g_d, g_a)[0]
    return AR.absgrad_reference(_FW[case], g_c, g_d, signed_want=want, g_a=g_a)[0]


MIN_T = 5e-3  # every pixel's final transmittance: far above the 1e-4 termination


def preconditions(O, case):
    """Assert what lets every element be compared: each tile lists all n Gaussians, no alpha or T decision lies in a
    flip band of oracle/parity.py (no flag), none is near its threshold in fp64 either, nothing terminates and the
    0.99 cap never binds."""
    from gpu_helpers import o_bounds
    W, H, n = case
    sc, r = scene(case), reference(O, case)
    ref, ex = r["ref"], r["export"]
    lens = (ex["ranges"][:, 1].astype(np.int64) - ex["ranges"][:, 0]).reshape(-1)
    assert len(lens) == ((W + 15) // 16) * ((H + 15) // 16) and (lens == n).all(), lens
    assert (r["radii"] > 0).all() and r["nr"] == n * len(lens)
    b = o_bounds(O, sc["s"], r["state"], r["radii"], upstream(O, case, "color")[0])
    assert int((np.asarray(b["gflag"]) != 0).sum()) == 0 and int((np.asarray(b["pflag"]) != 0).sum()) == 0
    assert ref["near_threshold"] == 0
    assert np.array_equal(ref["n_contrib"], ex["n_contrib"])
    assert ref["clamp099"] == 0 and ref["n_terminated"] == 0 and ref["min_T"] > MIN_T, ref["min_T"]
    assert ref["n_clamped"] == 0 and not ref["nonpd"].any()
    # every Gaussian blends somewhere: its record's sums are not all zero
    assert (np.abs(autograd_grads(O, case, *upstream(O, case, "color"))[2]) > 0).all()
