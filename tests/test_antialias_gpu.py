"""GPU tests of the opt-in antialiased rasterization (footprint-compensated opacity o_eff = o s,
s = sqrt(max(2.5e-5, det S / det(S + 0.3 I))); include/gs4d.h gs4d_forward_aa / gs4d_backward_aa).

  1. off is off: antialiasing=False through the new entries gives the existing entries' bytes
  2. the fold identity, bitwise: the antialiased forward equals the existing plain forward run at opacities = o_eff
     (read back with gs4d_debug_effective_opacity), and so do the gradients that do not pass through s.  This pins
     everything but s and its chain to code that is already tested.
  3. the factor: o_eff / o against the fp64 s per visible Gaussian, within 4 K32 kappa_i, where K32 is measured on
     a step-by-step numpy float32 restatement of computeCov3D / computeCov2D and the formula (never on the GPU) and
     kappa_i = (a0 c0 + b^2) / |D0|; the factor 4 because glm's column-major order and the restatement's may round
     differently.  Floored Gaussians give fl(sqrtf(2.5e-5f) o) to the last bit of the sqrtf.
  4. every gradient element against the fp64 restatement (tests/antialias_refs.py) within
     GRAD_RTOL |ref| + F max|ref|, F = max(GRAD_FLOOR, 2 F_oracle), the constants and the form of
     tests/test_rule_branches_gpu.py; F_oracle is the floor the fp32 oracle needs on the folded plain problem of
     the same scene (tests/antialias_scenes.oracle_floor_pairs, reference side only).  Images within IMG_ATOL.
  5. two runs with every option on are byte-equal
  6. render(), train_step and infer.render_view carry the switch

The scenes and the margins that make the comparison element-wise: tests/antialias_scenes.py,
tests/test_antialias_boundary.py.
"""
import math

import numpy as np
import pytest
import torch

import antialias_scenes as AS
from gpu_helpers import to_dev
from oracle import parity as PAR
from test_depth_grad_gpu import needed_floor
from test_rule_branches_gpu import _pairs, _ratio

pytestmark = pytest.mark.gpu

NAMES8 = PAR.GRAD_NAMES
# variant -> (upstream case, images passed, absgrad)
VARIANTS = {"colour": ("color", 1, False), "depth": ("both", 2, False), "aux": ("all", 3, False),
            "absgrad": ("all", 3, True)}
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _inputs(name):
    if name not in _GPU:
        sc = AS.scene(name)
        dev = torch.device("cuda:0")
        d = to_dev(sc["s"], dev)
        d["colors"] = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
        d["cov3D"] = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
        _GPU[name] = d
    return _GPU[name]


def forward(name, aa, opacities=None, entry="rasterize_gaussians_aa"):
    """a forward entry on the scene: (num_rendered, color, depth, radii, geom, binning, image buffers)"""
    sc, d = AS.scene(name), _inputs(name)
    s = sc["s"]
    e = torch.empty(0, device="cuda:0")
    cov = d["cov3D"]
    args = (d["bg"], d["means3D"], e if d["colors"] is None else d["colors"],
            d["opacities"] if opacities is None else opacities, e if cov is not None else d["scales"],
            e if cov is not None else d["rotations"], float(s["scale_modifier"]), e if cov is None else cov,
            d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]), int(s["H"]), int(s["W"]),
            d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], False, False)
    if entry == "rasterize_gaussians":
        return _C().rasterize_gaussians(*args)
    return _C().rasterize_gaussians_aa(*args, aa)


def backward(name, fwd, grads, entry="rasterize_gaussians_backward_aa", aa=True, absgrad=False):
    """a backward entry after `fwd`; grads = the upstream images (an empty or missing one = none)"""
    sc, d = AS.scene(name), _inputs(name)
    s = sc["s"]
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = fwd
    cov = d["cov3D"]
    imgs = [e if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda:0") for x in grads]
    if entry == "rasterize_gaussians_backward_aa":
        imgs += [e] * (3 - len(imgs))
    args = (d["bg"], d["means3D"], radii, e if d["colors"] is None else d["colors"],
            e if cov is not None else d["scales"], e if cov is not None else d["rotations"],
            float(s["scale_modifier"]), e if cov is None else cov, d["viewmatrix"], d["projmatrix"],
            float(s["tanfovx"]), float(s["tanfovy"]), *imgs, d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]),
            d["campos"], gb, nr, bb, ib, False)
    if entry == "rasterize_gaussians_backward_aa":
        return _C().rasterize_gaussians_backward_aa(*args, d["opacities"], aa, absgrad)
    return getattr(_C(), entry)(*args)


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        if torch.is_tensor(x):
            assert x.shape == y.shape and torch.equal(x, y), f"{what}: output {i} differs"
        else:
            assert x == y, f"{what}: output {i} differs"


# ---- 1. off is off ---------------------------------------------------------------------------------------------
def test_off_is_the_existing_entries_bits(oracle):
    name = "aa_mid"
    ups = AS.upstream(oracle, name, "all")
    old = forward(name, False, entry="rasterize_gaussians")
    new = forward(name, False)
    _same(old[:4], new[:4], "forward")
    assert torch.equal(_C().alpha_image(old[6], 45, 70), _C().alpha_image(new[6], 45, 70))
    assert torch.equal(_C().debug_effective_opacity(new[4], 200)[new[3] > 0],
                       _inputs(name)["opacities"][:, 0][new[3] > 0])
    want = backward(name, old, ups, entry="rasterize_gaussians_backward_absgrad")
    got = backward(name, new, ups, aa=False, absgrad=True)
    _same(want, got, "backward, every option on")
    assert len(got) == 9 and got[3].abs().max() > 0 and got[8].abs().max() > 0
    # and each narrower combination against its own entry
    for entry, n_img in (("rasterize_gaussians_backward", 1), ("rasterize_gaussians_backward_depth", 2),
                         ("rasterize_gaussians_backward_aux", 3)):
        want = backward(name, old, ups[:n_img], entry=entry)
        got = backward(name, new, ups[:n_img], aa=False, absgrad=False)
        _same(want, got[:8], entry)
        assert got[8].numel() == 0


# ---- 2. the fold identity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AS.NAMES)
def test_fold_identity_is_bitwise(oracle, name):
    s = AS.scene(name)["s"]
    H, W, P = int(s["H"]), int(s["W"]), s["means3D"].shape[0]
    d = _inputs(name)
    aa = forward(name, True)
    radii = aa[3]
    o_eff = _C().debug_effective_opacity(aa[4], P)
    assert o_eff.shape == (P,) and int((radii > 0).sum()) >= 50
    o_fold = torch.where(radii > 0, o_eff, d["opacities"][:, 0]).reshape(P, 1).contiguous()
    assert (o_fold[radii > 0] < d["opacities"][radii > 0]).all()       # the factor is below 1 ...
    plain = forward(name, False, opacities=o_fold, entry="rasterize_gaussians")
    _same(aa[:4], plain[:4], "forward")                                 # num_rendered, colour, depth, radii
    assert torch.equal(_C().alpha_image(aa[6], H, W), _C().alpha_image(plain[6], H, W))
    off = forward(name, False)
    assert torch.equal(off[3], radii) and off[0] == aa[0]               # ... and moves neither radii nor the count
    assert not torch.equal(off[1], aa[1])
    ups = AS.upstream(oracle, name, "all")
    g_aa = backward(name, aa, ups, aa=True, absgrad=True)
    g_pl = backward(name, plain, ups, entry="rasterize_gaussians_backward_absgrad")
    for i in (0, 1, 5, 8):                                              # dL_dmeans2D, dL_dcolors, dL_dsh, absgrad
        assert torch.equal(g_aa[i], g_pl[i]), f"{NAMES8[i] if i < 8 else 'absgrad'} differs from the folded problem"
    assert g_aa[0].abs().max() > 0 and g_aa[8].abs().max() > 0
    # what passes through s is not the folded problem's
    assert not torch.equal(g_aa[2], g_pl[2]) and not torch.equal(g_aa[3], g_pl[3])


# ---- 3. the factor ---------------------------------------------------------------------------------------------
def _mul32(A, B):
    """(P, 3, 3) float32 product, each entry summed in k order with float32 roundings (glm's operator*)"""
    out = np.empty_like(A)
    for r in range(3):
        for c in range(3):
            out[:, r, c] = (A[:, r, 0] * B[:, 0, c] + A[:, r, 1] * B[:, 1, c]) + A[:, r, 2] * B[:, 2, c]
    return out


def numpy32_effective_opacity(sc):
    """computeCov3D, computeCov2D (forward.cu:74-152) and the formula in numpy float32, operation by operation;
    matrices are held as math matrices A[row][col] (= glm's m[col][row]).  Returns fl(o s) / o as float64 (P,)."""
    f = np.float32
    s = sc["s"]
    P = s["means3D"].shape[0]
    if sc["cov3D"] is not None:
        c6 = sc["cov3D"].astype(f)
    else:
        sc3 = f(s["scale_modifier"]) * s["scales"].astype(f)
        q = s["rotations"].astype(f)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, two = f(1), f(2)
        R = np.zeros((P, 3, 3), f)   # quat_mat's columns are the rows of the usual rotation matrix
        R[:, 0, 0], R[:, 1, 0], R[:, 2, 0] = one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)
        R[:, 0, 1], R[:, 1, 1], R[:, 2, 1] = two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)
        R[:, 0, 2], R[:, 1, 2], R[:, 2, 2] = two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)
        S = np.zeros((P, 3, 3), f)
        S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = sc3[:, 0], sc3[:, 1], sc3[:, 2]
        M = _mul32(S, R)
        Sig = _mul32(np.ascontiguousarray(M.transpose(0, 2, 1)), M)
        c6 = np.stack([Sig[:, 0, 0], Sig[:, 1, 0], Sig[:, 2, 0], Sig[:, 1, 1], Sig[:, 2, 1], Sig[:, 2, 2]], 1)
    v = s["viewmatrix"].astype(f).reshape(-1)
    m = s["means3D"].astype(f)
    t = [((v[i] * m[:, 0] + v[4 + i] * m[:, 1]) + v[8 + i] * m[:, 2]) + v[12 + i] for i in range(3)]
    tfx, tfy = f(s["tanfovx"]), f(s["tanfovy"])
    fx, fy = f(s["W"]) / (f(2) * tfx), f(s["H"]) / (f(2) * tfy)
    limx, limy = f(1.3) * tfx, f(1.3) * tfy
    tz = t[2]
    tx = np.minimum(limx, np.maximum(-limx, t[0] / tz)) * tz
    ty = np.minimum(limy, np.maximum(-limy, t[1] / tz)) * tz
    J = np.zeros((P, 3, 3), f)
    J[:, 0, 0], J[:, 2, 0] = fx / tz, -(fx * tx) / (tz * tz)
    J[:, 1, 1], J[:, 2, 1] = fy / tz, -(fy * ty) / (tz * tz)
    Wm = np.broadcast_to(np.array([[v[0], v[1], v[2]], [v[4], v[5], v[6]], [v[8], v[9], v[10]]], f), (P, 3, 3)).copy()
    T = _mul32(Wm, J)
    V = np.stack([np.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), np.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                  np.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)
    cov = _mul32(_mul32(np.ascontiguousarray(T.transpose(0, 2, 1)), np.ascontiguousarray(V.transpose(0, 2, 1))), T)
    a0, b, c0 = cov[:, 0, 0], cov[:, 1, 0], cov[:, 1, 1]
    a, c = a0 + f(0.3), c0 + f(0.3)
    D0 = a0 * c0 - b * b
    D1 = a * c - b * b
    r = D0 / D1
    sfac = np.sqrt(np.maximum(f(2.5e-5), r))
    o = s["opacities"].astype(f)[:, 0]
    assert (o * sfac).dtype == np.float32
    return (o * sfac).astype(np.float64) / o.astype(np.float64)


@pytest.mark.parametrize("name", AS.NAMES)
def test_factor_matches_fp64_within_the_float32_bound(oracle, name):
    sc, r = AS.scene(name), AS.reference(oracle, name)
    P = sc["s"]["means3D"].shape[0]
    fwd = forward(name, True)
    vis = (fwd[3] > 0).cpu().numpy()
    assert np.array_equal(vis, r["radii"] > 0)
    o = sc["s"]["opacities"][:, 0].astype(np.float64)
    got = _C().debug_effective_opacity(fwd[4], P).cpu().numpy().astype(np.float64) / o
    s64, kappa, floored = r["s64"], r["kappa"], r["floored"]
    rows = vis & ~floored
    rel32 = np.abs(numpy32_effective_opacity(sc) - s64) / s64
    K32 = float((rel32[rows] / kappa[rows]).max())
    assert 0 < K32 < 1e-6, K32     # float32's rounding unit is 6e-8: the restatement is a float32 computation
    ratio = np.abs(got - s64)[rows] / s64[rows] / (4.0 * K32 * kappa[rows])
    print(f"[aa-factor] {name}: K32 = {K32:.3e}, kappa max {kappa[rows].max():.1f}, worst GPU "
          f"|o_eff / o - s| / (4 K32 kappa s) = {ratio.max():.3f}, floored {int((vis & floored).sum())}", flush=True)
    assert ratio.max() <= 1.0
    if floored.any():
        s_floor = np.sqrt(np.float32(2.5e-5))
        o32 = sc["s"]["opacities"][:, 0].astype(np.float32)
        allowed = [(o32 * x).astype(np.float64) / o for x in
                   (np.nextafter(s_floor, np.float32(0)), s_floor, np.nextafter(s_floor, np.float32(1)))]
        fr = vis & floored
        assert fr.sum() >= 8
        assert np.all((got[fr] == allowed[0][fr]) | (got[fr] == allowed[1][fr]) | (got[fr] == allowed[2][fr]))


# ---- 4. gradients against fp64 ---------------------------------------------------------------------------------
_FLOOR = {}


def floors(O, name):
    """(F_oracle, F) of the scene, from the oracle and the restatement on the folded plain problem alone"""
    if name not in _FLOOR:
        got, want, radii, _ = AS.oracle_floor_pairs(O, name)
        f_oracle = needed_floor(_pairs(got, want, radii))
        _FLOOR[name] = (f_oracle, max(PAR.GRAD_FLOOR, 2.0 * f_oracle))
    return _FLOOR[name]


@pytest.mark.parametrize("name", AS.NAMES)
def test_forward_images_match_fp64(oracle, name):
    r = AS.reference(oracle, name)
    s, ref = AS.scene(name)["s"], r["ref"]
    nr, color, depth, radii = forward(name, True)[:4]
    assert nr == r["nr"] and np.array_equal(radii.cpu().numpy(), r["radii"])
    alpha = _C().alpha_image(forward(name, True)[6], int(s["H"]), int(s["W"]))
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    e_c = float(np.abs(f64(color) - ref["color"].detach().numpy()).max())
    e_d = float(np.abs(f64(depth) - ref["depth"].detach().numpy()).max())
    e_a = float(np.abs(f64(alpha)[0] - (1.0 - ref["Tfinal"].detach().numpy())).max())
    print(f"[aa-forward] {name}: max |gpu - fp64| colour {e_c:.3e} depth {e_d:.3e} alpha {e_a:.3e} "
          f"(bar {PAR.IMG_ATOL})", flush=True)
    assert e_c <= PAR.IMG_ATOL and e_d <= PAR.IMG_ATOL and e_a <= PAR.IMG_ATOL


@pytest.mark.parametrize("name", AS.NAMES)
def test_backward_matches_fp64(oracle, name):
    """every element of every gradient of the antialiased backward within GRAD_RTOL |ref| + F max|ref| of the fp64
    restatement; all four variants on aa_small, colour and aux on the others (the measured ratios: DESIGN 10.11)"""
    f_oracle, F = floors(oracle, name)
    fwd = forward(name, True)
    radii = fwd[3].cpu().numpy()
    assert np.array_equal(radii, AS.reference(oracle, name)["radii"])
    variants = list(VARIANTS) if name == "aa_small" else ["colour", "aux"]
    failures = []
    for var in variants:
        case, n_img, absgrad = VARIANTS[var]
        ups = AS.upstream(oracle, name, case)
        got = backward(name, fwd, ups[:n_img], aa=True, absgrad=absgrad)
        assert len(got) == 9 and (got[8].numel() > 0) == absgrad
        pairs = _pairs(got[:8], AS.autograd_grads(oracle, name, *ups), radii)
        assert [n for n, _, _ in pairs][:5] == NAMES8[:5]
        if AS.scene(name)["cov3D"] is None:
            assert [n for n, _, _ in pairs][-2:] == NAMES8[-2:]      # dL_dscales, dL_drotations
        worst = {n: _ratio(a, b, F) for n, a, b in pairs}
        assert got[2].abs().max() > 0 and got[3].abs().max() > 0 and got[4].abs().max() > 0
        if absgrad:
            absg = got[8].cpu().numpy()
            assert np.isfinite(absg).all() and not np.any(absg[:, 2]) and not np.any(absg[radii == 0])
            assert np.all(absg >= 0) and absg.max() > 0
        print(f"[aa-parity] {name} {var}: F_oracle = {f_oracle:.3e}, F = {F:.3e}; worst ratios "
              + " ".join(f"{n}={v:.3f}" for n, v in worst.items()), flush=True)
        failures += [f"{var} {n}: an element off by {v:.2f}x its bar ({PAR.GRAD_RTOL} |ref| + {F:.2e} max|ref|)"
                     for n, v in worst.items() if not v <= 1.0]
    assert not failures, "; ".join(failures)


def test_floored_gaussians_get_an_opacity_gradient_and_none_through_s(oracle):
    """aa_floor: on the floored rows dL/do = g s is not zero, and the scale / rotation gradients are exactly those
    of the folded plain problem (dL/dr = 0: nothing is added to the conic's own terms)"""
    name = "aa_floor"
    r = AS.reference(oracle, name)
    ups = AS.upstream(oracle, name, "all")
    aa = forward(name, True)
    P = len(r["radii"])
    o_eff = _C().debug_effective_opacity(aa[4], P)
    o_fold = torch.where(aa[3] > 0, o_eff, _inputs(name)["opacities"][:, 0]).reshape(P, 1).contiguous()
    plain = forward(name, False, opacities=o_fold, entry="rasterize_gaussians")
    g_aa = backward(name, aa, ups, aa=True)
    g_pl = backward(name, plain, ups, entry="rasterize_gaussians_backward_aux")
    rows = torch.tensor(r["floored"] & r["ref"]["blends"], device="cuda:0")
    assert int(rows.sum()) >= 8
    assert (g_aa[2][rows] != 0).all()
    for i in (4, 6, 7):
        assert torch.equal(g_aa[i][rows], g_pl[i][rows]), NAMES8[i]
    others = torch.tensor((r["radii"] > 0) & ~r["floored"], device="cuda:0")
    assert not torch.equal(g_aa[6][others], g_pl[6][others])


# ---- 5. determinism and composition ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aa_small", "aa_floor"])
def test_every_option_on_is_bitwise_repeatable(oracle, name):
    ups = AS.upstream(oracle, name, "all")
    runs = []
    for _ in range(2):
        fwd = forward(name, True)
        runs.append((fwd[:4], backward(name, fwd, ups, aa=True, absgrad=True)))
    _same(runs[0][0], runs[1][0], "forward")
    _same(runs[0][1], runs[1][1], "backward")
    assert runs[0][1][3].abs().max() > 0


# ---- 6. above the C boundary -----------------------------------------------------------------------------------
class _Canonical:
    """the least render() reads of a model at the coarse stage: raw parameters and their activations"""
    fused = False

    def __init__(self, s, dev):
        t = lambda a: torch.tensor(np.asarray(a), device=dev).requires_grad_(True)
        self._xyz = t(s["means3D"])
        self._scaling = t(np.log(s["scales"]))
        self._rotation = t(s["rotations"])
        o = s["opacities"].astype(np.float64)
        self._opacity = t(np.log(o / (1 - o)).astype(np.float32))
        self._shs = t(s["shs"])
        self.active_sh_degree = int(s["sh_degree"])
        self.scaling_activation = torch.exp
        self.rotation_activation = torch.nn.functional.normalize
        self.opacity_activation = torch.sigmoid

    get_xyz = property(lambda self: self._xyz)
    get_features = property(lambda self: self._shs)


def test_render_carries_the_switch(oracle):
    from gs4d_train.render import render
    name = "aa_small"
    s = AS.scene(name)["s"]
    dev = torch.device("cuda:0")
    pc = _Canonical(s, dev)
    bg = torch.tensor(s["bg"], device=dev)
    on = render(s["camera"], pc, False, bg, stage="coarse", antialiasing=True, alpha=True)
    off = render(s["camera"], pc, False, bg, stage="coarse", alpha=True)
    assert torch.equal(on["radii"], off["radii"]) and not torch.equal(on["render"], off["render"])
    d_alpha = (off["alpha"] - on["alpha"]).detach()
    assert float(d_alpha.min()) >= -1e-6 and float(d_alpha.max()) > 0.05
    # the C-level forward on the activated tensors render() hands over
    d = dict(_inputs(name))
    with torch.no_grad():
        op, sc, rot = torch.sigmoid(pc._opacity), torch.exp(pc._scaling), torch.nn.functional.normalize(pc._rotation)
    cam = s["camera"]
    view_m, proj_m, cam_c = cam.on_device(dev) if hasattr(cam, "on_device") else (
        cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), cam.camera_center.to(dev))
    e = torch.empty(0, device=dev)
    want = _C().rasterize_gaussians_aa(bg, d["means3D"], e, op, sc, rot, 1.0, e, view_m, proj_m,
                                       math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), int(s["H"]), int(s["W"]),
                                       d["shs"], int(s["sh_degree"]), cam_c, False, False, True)
    assert torch.equal(on["render"], want[1]) and torch.equal(on["depth"], want[2])
    assert torch.equal(on["alpha"], _C().alpha_image(want[6], int(s["H"]), int(s["W"])))
    # and its backward is the C-level antialiased one: gradients arrive on every parameter, finite
    g = torch.Generator(device="cpu").manual_seed(3)
    g_c = torch.randn(on["render"].shape, generator=g).to(dev)
    (on["render"] * g_c).sum().backward()
    got = _C().rasterize_gaussians_backward_aa(
        bg, d["means3D"], want[3], e, sc, rot, 1.0, e, view_m, proj_m, math.tan(cam.FoVx * 0.5),
        math.tan(cam.FoVy * 0.5), g_c, e, e, d["shs"], int(s["sh_degree"]), cam_c, want[4], want[0], want[5], want[6],
        False, op, True, False)
    assert torch.equal(pc._xyz.grad, got[3]) and torch.equal(pc._shs.grad, got[5])
    assert torch.equal(on["viewspace_points"].grad, got[0])
    for p in (pc._opacity, pc._scaling, pc._rotation):
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0


def test_train_step_with_the_switch_on():
    """two iterations of the fused step with opt.antialiasing: every view rendered with antialiasing=True, a finite
    loss, and finite gradients on every parameter group that are not the switch-off step's"""
    import test_depth_grad_gpu as TD
    from gs4d_train import config
    from gs4d_train.render import render
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    W, H, P = 64, 48, 500
    pts, cols = make_point_cloud(P, seed=5)
    views = make_training_views(2, W, H, seed=6)
    bg = torch.ones(3, device="cuda")

    def run(flag, iters):
        hyper, opt = config.dynerf()
        opt.antialiasing = flag
        g = TD._train_model(pts, cols, opt, hyper)
        seen, out = [], []

        def render_fn(*a, **kw):
            seen.append(kw.get("antialiasing"))
            return render(*a, **kw)
        grads = {}
        step = g.optimizer.step

        def recording_step(*a, **kw):  # the gradients as the optimizer finds them (the step then clears them)
            grads.update({n: p.grad.detach().clone() for n, p in g._deformation.named_parameters()
                          if p.grad is not None})
            for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
                grads[n] = getattr(g, n).grad.detach().clone()
            return step(*a, **kw)
        g.optimizer.step = recording_step
        for it in iters:
            grads.clear()
            loss = train_step(g, views, opt, hyper, it, bg, render_fn=render_fn)
            out.append((float(loss), dict(grads)))
        return seen, out

    seen, out = run(True, (3001, 3002))
    assert seen == [True] * 4
    for loss, grads in out:
        assert math.isfinite(loss) and len(grads) > 6
        for n, t in grads.items():
            assert torch.isfinite(t).all(), n
        for n in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"):
            assert grads[n].abs().max() > 0, n
    seen_off, out_off = run(False, (3001,))
    assert seen_off == [None] * 2
    assert out_off[0][0] != out[0][0] and not torch.equal(out_off[0][1]["_scaling"], out[0][1]["_scaling"])


def test_render_view_carries_the_switch():
    """infer.render_view(..., antialiasing=True) against render(..., antialiasing=True) under no_grad, with the bar
    tests/test_infer_gpu.py uses for that pair: mean |render_view - unfused render()| <= 2 d0 + 1e-6, d0 = mean
    |fused render() - unfused render()|; render_set and evaluate hand the switch to render_view"""
    import test_infer_gpu as TI
    from gs4d_train import infer
    from gs4d_train.render import render
    g = TI._shared_model("dnerf")
    cams = TI._cameras(3)
    cam = cams[1]
    bg = torch.ones(3, device="cuda")
    state = infer.prepare(g)
    pkg = infer.render_view(cam, state, bg, antialiasing=True)
    plain = infer.render_view(cam, state, bg)
    assert torch.equal(pkg["radii"], plain["radii"]) and not torch.equal(pkg["render"], plain["render"])
    net = g._deformation.deformation_net
    try:
        with torch.no_grad():
            fused_img = render(cam, g, False, bg, antialiasing=True)["render"]
            g.fused = net.grid.fused = net.fused_heads = False
            unfused_img = render(cam, g, False, bg, antialiasing=True)["render"]
    finally:
        g.fused = net.grid.fused = net.fused_heads = True
    d0 = float((fused_img - unfused_img).abs().mean())
    d1 = float((pkg["render"] - unfused_img).abs().mean())
    print(f"\n[aa-infer] render_view 64x48 antialiased: mean |render_view - unfused render()| = {d1:.3e}, d0 = {d0:.3e}")
    assert d1 <= 2 * d0 + 1e-6
    images, _ = infer.render_set(state, cams, bg, antialiasing=True)
    assert torch.equal(images[1], pkg["render"])
    gts = [(c, torch.rand(3, 48, 64, generator=torch.Generator().manual_seed(i))) for i, c in enumerate(cams)]
    m_on, m_off = infer.evaluate(state, gts, bg, antialiasing=True), infer.evaluate(state, gts, bg)
    assert math.isfinite(m_on["psnr"]) and m_on["psnr"] != m_off["psnr"]
