"""GPU tests of the rasterizer's rule-bound branches: the frustum clamp (Q22) with focal_x != focal_y, the scale
modifier (Q26), conics that are not positive definite (the blend kernels' general walk and its power > 0 skip), the
binding 0.99 cap (Q17) and the T < 1e-4 termination -- forward and all four backward entries.

Reference: the fp64 autograd restatement of those rules (tests/torch_restatement.py) on the scenes of
tests/rule_scenes.py, where each rule binds and no decision is near its threshold
(tests/test_rule_branches_boundary.py asserts the margins and pins the oracle to the restatement), so every element
of every tensor is compared; num_rendered and radii are compared exactly with the oracle.

The gradient bar has the form of the depth, alpha and absgrad suites, |gpu - ref| <= GRAD_RTOL |ref| + F max|ref| per
element, with F set per scene from the reference side alone: F = max(GRAD_FLOOR, 2 F_oracle), F_oracle the smallest
floor at which the fp32 ORACLE's colour backward meets that form against the fp64 colour gradients of the same scene
(computed here on the CPU).  The factor 2 is the margin the depth suite gives an fp32 sum in another order with one
more rounded term.
"""
import numpy as np
import pytest
import torch

import rule_scenes as RS
from gpu_helpers import c_forward, o_backward, to_dev
from oracle import parity as PAR
from test_depth_grad_gpu import needed_floor

pytestmark = pytest.mark.gpu

NAMES8 = PAR.GRAD_NAMES
# entry -> (the gradient images it takes, the upstream case of rule_scenes.upstream)
ENTRIES = {
    "rasterize_gaussians_backward": (1, "color"),
    "rasterize_gaussians_backward_depth": (2, "both"),
    "rasterize_gaussians_backward_aux": (3, "all"),
    "rasterize_gaussians_backward_absgrad": (3, "all"),
}
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def gpu_forward(name):
    """device tensors, the HIP forward and the alpha image of a scene, made once"""
    if name not in _GPU:
        sc = RS.scene(name)
        s = sc["s"]
        dev = torch.device("cuda:0")
        d = to_dev(s, dev)
        colors = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
        cov3D = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
        fwd = c_forward(_C(), s, d, colors=colors, cov3D=cov3D, use_sh=sc["use_sh"])
        alpha = _C().alpha_image(fwd[6], int(s["H"]), int(s["W"]))
        _GPU[name] = dict(d=d, colors=colors, cov3D=cov3D, fwd=fwd, alpha=alpha)
    return _GPU[name]


def backward(entry, name, grads):
    """a _C backward entry with the scene's tensors and the gradient images `grads` in the entry's order"""
    sc, g = RS.scene(name), gpu_forward(name)
    s, d = sc["s"], g["d"]
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = g["fwd"]
    cov = g["cov3D"]
    imgs = [torch.tensor(np.ascontiguousarray(x), device="cuda:0") for x in grads]
    return getattr(_C(), entry)(
        d["bg"], d["means3D"], radii, e if g["colors"] is None else g["colors"], e if cov is not None else d["scales"],
        e if cov is not None else d["rotations"], float(s["scale_modifier"]), e if cov is None else cov,
        d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), *imgs,
        d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], gb, nr, bb, ib, False)


def _pairs(got, want, radii):
    """(tensor name, array, fp64 reference) of the gradients the scene's input mode has; dL_dmeans2D's third column
    and every row of a culled Gaussian must be exactly zero"""
    out = []
    for n, a, b in zip(NAMES8, got, want):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if n == "dL_dmeans2D":
            assert not np.any(a[:, 2])
            a = a[:, :2]
        assert np.isfinite(a).all(), n
        assert not np.any(a.reshape(len(radii), -1)[radii == 0]) if a.size else True, f"{n}: culled rows not zero"
        if b is None or a.size == 0:
            continue
        out.append((n, a.astype(np.float64).reshape(b.shape), np.asarray(b, np.float64)))
    return out


_FLOOR = {}


def floors(O, name):
    """(F_oracle, F) of the scene, from the oracle and the restatement alone"""
    if name not in _FLOOR:
        sc, r = RS.scene(name), RS.reference(O, name)
        g_c, g_d, g_a = RS.upstream(O, name, "color")
        got = o_backward(O, sc["s"], r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"],
                         use_sh=sc["use_sh"])
        f_oracle = needed_floor(_pairs(got, RS.autograd_grads(O, name, g_c, g_d, g_a), r["radii"]))
        _FLOOR[name] = (f_oracle, max(PAR.GRAD_FLOOR, 2.0 * f_oracle))
    return _FLOOR[name]


def _ratio(a, b, F):
    """the largest |a - b| / (GRAD_RTOL |b| + F max|b|) over the elements"""
    scale = max(float(np.abs(b).max()), 1e-30)
    return float((np.abs(a - b) / (PAR.GRAD_RTOL * np.abs(b) + F * scale)).max())


@pytest.mark.parametrize("name", RS.NAMES)
def test_forward_matches_oracle_counts_and_fp64_images(oracle, name):
    r, g = RS.reference(oracle, name), gpu_forward(name)
    s, ref = RS.scene(name)["s"], r["ref"]
    nr, color, depth, radii = g["fwd"][:4]
    assert nr == r["nr"], f"num_rendered {nr} != oracle {r['nr']}"
    assert np.array_equal(radii.cpu().numpy(), r["radii"]), "radii differ"
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    e_c = float(np.abs(f64(color) - ref["color"].detach().numpy()).max())
    e_d = float(np.abs(f64(depth) - ref["depth"].detach().numpy()).max())
    assert g["alpha"].shape == (1, s["H"], s["W"])
    e_a = float(np.abs(f64(g["alpha"])[0] - (1.0 - ref["Tfinal"].detach().numpy())).max())
    print(f"[rule-forward] {name}: max |gpu - fp64| colour {e_c:.3e} depth {e_d:.3e} alpha {e_a:.3e} "
          f"(bar {PAR.IMG_ATOL})", flush=True)
    assert e_c <= PAR.IMG_ATOL and e_d <= PAR.IMG_ATOL and e_a <= PAR.IMG_ATOL


@pytest.mark.parametrize("name", RS.NAMES)
def test_backward_entries_match_fp64(oracle, name):
    f_oracle, F = floors(oracle, name)
    radii = gpu_forward(name)["fwd"][3].cpu().numpy()
    assert np.array_equal(radii, RS.reference(oracle, name)["radii"])
    failures = []
    for entry, (n_img, case) in ENTRIES.items():
        ups = RS.upstream(oracle, name, case)
        got = backward(entry, name, ups[:n_img])
        pairs = _pairs(got[:8], RS.autograd_grads(oracle, name, *ups), radii)
        assert [n for n, _, _ in pairs][:5] == NAMES8[:5]
        worst = {n: _ratio(a, b, F) for n, a, b in pairs}
        assert got[2].abs().max() > 0 and got[3].abs().max() > 0
        if entry.endswith("absgrad"):
            assert len(got) == 9
            absg = got[8].cpu().numpy().astype(np.float64)
            assert np.isfinite(absg).all() and not np.any(absg[:, 2]) and not np.any(absg[radii == 0])
            want = RS.absgrad(oracle, name, *ups)
            assert np.all(absg >= 0) and want.max() > 0
            worst["absgrad"] = _ratio(absg[:, :2], want, F)
        else:
            assert len(got) == 8
        print(f"[rule-parity] {name} {entry.replace('rasterize_gaussians_', '')}: F_oracle = {f_oracle:.3e}, "
              f"F = {F:.3e}; worst ratios " + " ".join(f"{n}={v:.3f}" for n, v in worst.items()), flush=True)
        failures += [f"{entry} {n}: an element off by {v:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"
                     for n, v in worst.items() if not v <= 1.0]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("name", RS.NAMES)
def test_backward_entries_are_bitwise_repeatable(oracle, name):
    for entry, (n_img, case) in ENTRIES.items():
        ups = RS.upstream(oracle, name, case)[:n_img]
        a, b = backward(entry, name, ups), backward(entry, name, ups)
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (entry, i)
        assert a[3].abs().max() > 0
