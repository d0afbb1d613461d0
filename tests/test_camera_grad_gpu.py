"""GPU tests of the opt-in camera gradient (include/gs4d.h gs4d_backward_camera).

  1. parity: each of the 35 elements of dL/dviewmatrix, dL/dprojmatrix, dL/dcampos within
     GRAD_RTOL A[k] + GRAD_FLOOR max_k A[k] of the fp64 graph (tests/camera_grad_refs.py), A[k] the mass of the
     per-Gaussian terms of element k: on the five scenes with the colour gradient, and on cam_sh and cam_colors with
     each of depth_grad, alpha, absgrad, antialiasing and with all of them
  2. bits: in every one of those calls the eight other gradients and absgrad are byte-equal to the option-off call
     (_C.rasterize_gaussians_backward_aa on the same forward), and a second call gives the same 35 floats
  3. the translation identity on the GPU's own outputs
  4. the reduction's edges: a 32 x 32 image, P = 0, 1 and every boundary of the two kernels' blocking +- 1, and P
     needing three rows and more, with colors_precomp (workgroups of 256) and with SHs (workgroups of 128)
  5. pose recovery on synthetic.bouncing_balls, and train_step with a PoseRefiner

That the parity bar bites (every family of terms is at least ten bars large somewhere) and the scenes' margins are
asserted on the CPU: tests/test_camera_grad_boundary.py.
"""
import math

import numpy as np
import pytest
import torch

import camera_grad_refs as CR
from gpu_helpers import o_forward, to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu

# variant -> (upstream case, (depth image, alpha image) passed, antialiasing, absgrad)
VARIANTS = {"colour": ("color", (False, False), False, False), "depth": ("both", (True, False), False, False),
            "alpha": ("all", (False, True), False, False), "absgrad": ("color", (False, False), False, True),
            "antialiasing": ("color", (False, False), True, False), "all": ("all", (True, True), True, True)}
_GPU = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _dev_scene(sc):
    dev = torch.device("cuda:0")
    d = to_dev(sc["s"], dev)
    d["colors"] = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
    return d


def _inputs(name):
    if name not in _GPU:
        _GPU[name] = _dev_scene(CR.scene(name))
    return _GPU[name]


def forward(sc, d, aa):
    s = sc["s"]
    e = torch.empty(0, device="cuda:0")
    return _C().rasterize_gaussians_aa(
        d["bg"], d["means3D"], e if d["colors"] is None else d["colors"], d["opacities"], d["scales"], d["rotations"],
        float(s["scale_modifier"]), e, d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]),
        int(s["H"]), int(s["W"]), d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], False, False, aa)


def backward(sc, d, fwd, grads, aa, absgrad, camera=True):
    """the camera entry (12 outputs) or, camera=False, the option-off call on the same forward (9 outputs)"""
    s = sc["s"]
    e = torch.empty(0, device="cuda:0")
    nr, color, depth, radii, gb, bb, ib = fwd
    imgs = [e if x is None else torch.tensor(np.ascontiguousarray(x), device="cuda:0") for x in grads]
    args = (d["bg"], d["means3D"], radii, e if d["colors"] is None else d["colors"], d["scales"], d["rotations"],
            float(s["scale_modifier"]), e, d["viewmatrix"], d["projmatrix"], float(s["tanfovx"]), float(s["tanfovy"]),
            *imgs, d["shs"] if sc["use_sh"] else e, int(s["sh_degree"]), d["campos"], gb, nr, bb, ib, False,
            d["opacities"], aa, absgrad)
    entry = _C().rasterize_gaussians_backward_camera if camera else _C().rasterize_gaussians_backward_aa
    return entry(*args)


def camera35(out):
    return torch.cat([out[9].reshape(-1), out[10].reshape(-1), out[11].reshape(-1)]).cpu().numpy().astype(np.float64)


def check_parity(tag, got35, cr):
    """worst |gpu - fp64| / bar per tensor; the assertion is per element"""
    bar = CR.bar(cr["A"])
    ratio = np.abs(got35 - cr["grad"]) / bar
    worst = {n: float(ratio[sl].max()) for n, sl in (("dV", slice(0, 16)), ("dPm", slice(16, 32)), ("dc", slice(32, 35)))}
    print(f"[camera-parity] {tag}: worst |gpu - fp64| / bar " + " ".join(f"{n}={v:.4f}" for n, v in worst.items())
          + f"; max A {cr['A'].max():.3e}", flush=True)
    # viewmatrix column 3 and projmatrix column 2 have no term at all (campos neither, without SHs): exact zeros
    zero = np.array([k < 16 and k % 4 == 3 or 16 <= k < 32 and k % 4 == 2 for k in range(35)])
    zero[32:] = not np.any(cr["A"][32:])
    assert not np.any(cr["A"][zero]) and not np.any(got35[zero]), f"{tag}: an element without terms is not zero"
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert bad.size == 0, f"{tag}: elements {bad.tolist()} off by {ratio[bad].max():.2f}x their bar"
    return worst


def check_translation(tag, sc, got, cr, radii):
    """sum_j dV[3, j] V[a, j] + sum_j dPm[3, j] Pm[a, j] - dc[a] = sum_i dL/dmeans3D_i[a] on the GPU's outputs, within
    the elements' bars carried through the identity's coefficients plus the means' own parity bar, summed"""
    V = sc["s"]["viewmatrix"].astype(np.float64).reshape(4, 4)
    Pm = sc["s"]["projmatrix"].astype(np.float64).reshape(4, 4)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    dV, dPm, dc, dm = f64(got[9]), f64(got[10]), f64(got[11]), f64(got[3])
    lhs, rhs = CR.translation_residual(V, Pm, dV, dPm, dc, dm)
    bar35 = CR.bar(cr["A"])
    ref_dm = cr["dmeans"]
    bar = np.abs(V[:3, :]) @ bar35[12:16] + np.abs(Pm[:3, :]) @ bar35[28:32] + bar35[32:35] + \
        PAR.GRAD_RTOL * np.abs(ref_dm).sum(0) + PAR.GRAD_FLOOR * np.abs(ref_dm).max() * int((radii > 0).sum())
    print(f"[camera-translation] {tag}: |lhs - rhs| / bar = {(np.abs(lhs - rhs) / bar).max():.4f}, "
          f"|rhs| max {np.abs(rhs).max():.3e}", flush=True)
    assert np.all(np.abs(lhs - rhs) <= bar)


def run_variant(oracle, name, var):
    case, (use_d, use_a), aa, absgrad = VARIANTS[var]
    sc, d = CR.scene(name), _inputs(name)
    g_c, g_d, g_a = CR.upstream(oracle, name, case)
    grads = (g_c, g_d if use_d else None, g_a if use_a else None)
    zeros = lambda g, used: g if used else np.zeros_like(g)
    ref = CR.reference(oracle, name, aa)
    cr = CR.camera_reference(ref["ref"], g_c, zeros(g_d, use_d), zeros(g_a, use_a))
    fwd = forward(sc, d, aa)
    radii = fwd[3].cpu().numpy()
    assert fwd[0] == ref["nr"] and np.array_equal(radii, ref["radii"])
    got = backward(sc, d, fwd, grads, aa, absgrad)
    off = backward(sc, d, fwd, grads, aa, absgrad, camera=False)
    assert len(got) == 12 and len(off) == 9
    assert got[9].shape == (4, 4) and got[10].shape == (4, 4) and got[11].shape == (3,)
    for i in range(9):   # the eight gradients and absgrad: the option-off call's bytes
        assert got[i].shape == off[i].shape and torch.equal(got[i], off[i]), f"{name} {var}: output {i} differs"
    assert (got[8].numel() > 0) == absgrad and got[3].abs().max() > 0
    again = backward(sc, d, fwd, grads, aa, absgrad)
    for i in (9, 10, 11):
        assert torch.equal(got[i].view(torch.int32), again[i].view(torch.int32)), f"{name} {var}: not repeatable"
    worst = check_parity(f"{name} {var}", camera35(got), cr)
    check_translation(f"{name} {var}", sc, got, cr, radii)
    return worst


# ---- 1-3. parity, bits, translation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.NAMES)
def test_camera_gradient_matches_fp64(oracle, name):
    run_variant(oracle, name, "colour")


@pytest.mark.parametrize("var", [v for v in VARIANTS if v != "colour"])
@pytest.mark.parametrize("name", ["cam_sh", "cam_colors"])
def test_camera_gradient_composes_with_the_other_options(oracle, name, var):
    run_variant(oracle, name, var)


def test_dense_scene_finishes_sums_inside_the_per_gaussian_kernel():
    """cam_dense is there for the Gaussians whose records straddle two waves of the reduction: count them from the
    forward's own lists"""
    sc, d = CR.scene("cam_dense"), _inputs("cam_dense")
    s = sc["s"]
    fwd = forward(sc, d, False)
    P = s["means3D"].shape[0]
    lists = _C().debug_tile_lists(fwd[4], fwd[5], fwd[6], P, int(s["W"]), int(s["H"]), fwd[0])
    gid, slot = lists[3].cpu().numpy(), lists[5].cpu().numpy()
    first = np.full(P, 2 ** 31 - 1, np.int64)
    last = np.full(P, -1, np.int64)
    np.minimum.at(first, gid, slot)
    np.maximum.at(last, gid, slot)
    straddling = int(((last >= 0) & (first // 64 != last // 64)).sum())
    print(f"[camera-dense] {lists[2]} instances, {straddling} Gaussians straddle two waves", flush=True)
    # the emitted instances fill about ten waves, so at most nine Gaussians can straddle; a third of that is asked
    assert lists[2] > 3 * 64 and straddling >= 3


def test_culled_third_adds_nothing(oracle):
    """cam_behind: a third of the Gaussians is behind the near plane (radii 0); moving them changes no bit"""
    sc, d = CR.scene("cam_behind"), dict(_inputs("cam_behind"))
    g_c = CR.upstream(oracle, "cam_behind", "color")[0]
    fwd = forward(sc, d, False)
    radii = fwd[3].cpu().numpy()
    assert int((radii[::3] == 0).sum()) == len(radii[::3]) and int((radii > 0).sum()) >= 30
    got = backward(sc, d, fwd, (g_c, None, None), False, False)
    m = d["means3D"].clone()
    V = torch.tensor(sc["s"]["viewmatrix"].reshape(4, 4)[:3, :3], device="cuda:0")
    m[::3] -= 0.5 * V[:, 2]          # further behind, along the view direction
    d["means3D"] = m
    fwd2 = forward(sc, d, False)
    assert torch.equal(fwd2[3], fwd[3])
    got2 = backward(sc, d, fwd2, (g_c, None, None), False, False)
    for i in (9, 10, 11):
        assert torch.equal(got[i], got2[i])


# ---- 4. the reduction's edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["colors", "sh"])
@pytest.mark.parametrize("P", CR.EDGE_P)
def test_reduction_edges(oracle, P, mode):
    """unit upstream gradients; the workgroups are 256 threads with colors_precomp and 128 with SHs, so these P put
    the last Gaussian at the end of a wave, of a workgroup, and one past each, and 700 leaves 3 and 6 rows"""
    sc = CR.edge_scene(P, mode)
    d = _dev_scene(sc)
    s = sc["s"]
    g_c = np.ones((3, 32, 32), np.float32)
    z = np.zeros((1, 32, 32), np.float32)
    ref = CR.make_reference(oracle, sc)
    cr = CR.camera_reference(ref["ref"], g_c, z, z)
    fwd = forward(sc, d, False)
    assert fwd[0] == ref["nr"] and np.array_equal(fwd[3].cpu().numpy(), ref["radii"])
    got = backward(sc, d, fwd, (g_c, None, None), False, False)
    again = backward(sc, d, fwd, (g_c, None, None), False, False)
    for i in (9, 10, 11):
        assert torch.equal(got[i].view(torch.int32), again[i].view(torch.int32))
    if cr["A"].max() == 0:      # nothing visible: 35 zeros
        assert not np.any(camera35(got))
        return
    check_parity(f"edge P={P} {mode}", camera35(got), cr)
    check_translation(f"edge P={P} {mode}", sc, got, cr, ref["radii"])


def test_no_gaussians_and_no_instances_give_35_zeros():
    dev = torch.device("cuda:0")
    e = torch.empty(0, device=dev)
    f = lambda *shape: torch.zeros(*shape, device=dev)
    eye = torch.eye(4, device=dev)
    # P = 0
    fwd = _C().rasterize_gaussians_aa(torch.ones(3, device=dev), f(0, 3), e, f(0, 1), f(0, 3), f(0, 4), 1.0, e, eye, eye,
                                      0.5, 0.5, 32, 32, f(0, 16, 3), 3, f(3), False, False, False)
    out = _C().rasterize_gaussians_backward_camera(
        torch.ones(3, device=dev), f(0, 3), fwd[3], e, f(0, 3), f(0, 4), 1.0, e, eye, eye, 0.5, 0.5,
        torch.ones(3, 32, 32, device=dev), e, e, f(0, 16, 3), 3, f(3), fwd[4], fwd[0], fwd[5], fwd[6], False, f(0, 1),
        False, False)
    assert len(out) == 12 and out[3].shape == (0, 3)
    for i in (9, 10, 11):
        assert not out[i].any() and out[i].numel() in (16, 3)
    # P = 3, all of them far outside the frustum: num_rendered = 0
    from gs4d_train.synthetic import make_scene
    s = make_scene(3, 32, 32, seed=1)
    s["means3D"][:, 0] += 500.0
    sc = dict(s=s, colors=None, use_sh=True)
    d = _dev_scene(sc)
    fwd = forward(sc, d, False)
    assert fwd[0] == 0
    got = backward(sc, d, fwd, (np.ones((3, 32, 32), np.float32), None, None), False, False)
    assert not np.any(camera35(got)) and not got[3].any()


# ---- the Python layers -----------------------------------------------------------------------------------------
class _Canonical:
    """the least render() reads of a model at the coarse stage: raw parameters and their activations"""
    fused = False

    def __init__(self, s, dev, requires_grad=True):
        t = lambda a: torch.tensor(np.asarray(a), device=dev).requires_grad_(requires_grad)
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


def test_render_hands_the_gradients_to_the_tensors_that_ask(oracle):
    """render(camera_grad=True, camera_tensors=...): the leaves that require grad get the C entry's gradients, the
    Gaussians' gradients are the flag-off call's bits, and a leaf that does not require grad gets none"""
    from gs4d_train.render import render
    name = "cam_sh"
    s = CR.scene(name)["s"]
    dev = torch.device("cuda:0")
    bg = torch.tensor(s["bg"], device=dev)
    cam = s["camera"]
    g_c = torch.tensor(CR.upstream(oracle, name, "color")[0], device=dev)
    V0, Pm0, c0 = cam.on_device(dev)

    def run(camera_grad, leaves):
        pc = _Canonical(s, dev)
        kw = {}
        if leaves is not None:
            kw = dict(camera_grad=camera_grad, camera_tensors=leaves)
        pkg = render(cam, pc, False, bg, stage="coarse", **kw)
        (pkg["render"] * g_c).sum().backward()
        return pkg, pc

    V = V0.clone().requires_grad_(True)
    Pm = Pm0.clone().requires_grad_(True)
    c = c0.clone()                                     # does not ask
    on, pc_on = run(True, (V, Pm, c))
    off, pc_off = run(False, None)
    assert torch.equal(on["render"], off["render"]) and torch.equal(on["radii"], off["radii"])
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_shs"):
        assert torch.equal(getattr(pc_on, n).grad, getattr(pc_off, n).grad), n
    assert torch.equal(on["viewspace_points"].grad, off["viewspace_points"].grad)
    assert V.grad is not None and Pm.grad is not None and c.grad is None
    cr = CR.camera_ref(oracle, name, "color")
    # render() activates the raw parameters itself (exp(log(scale)) ...), which are not bit for bit the scene's
    # arrays: the bar of the parity test is kept and the inputs' rounding, one ulp of each, is far inside it
    got = np.concatenate([V.grad.reshape(-1).cpu().numpy(), Pm.grad.reshape(-1).cpu().numpy()]).astype(np.float64)
    ratio = np.abs(got - cr["grad"][:32]) / CR.bar(cr["A"])[:32]
    print(f"[camera-render] worst |render()'s gradient - fp64| / bar = {ratio.max():.4f}", flush=True)
    assert ratio.max() <= 1.0
    # without camera_grad the same tensors are plain inputs
    V2 = V0.clone().requires_grad_(True)
    run(False, (V2, Pm0, c0))
    assert V2.grad is None


def _pose_problem(seed):
    """bouncing_balls at t = 0.3 seen from 3 units away, 96 x 72; the ground truth is the oracle's rendering"""
    from gs4d_train.synthetic import bouncing_balls, look_at_camera
    from oracle import oracle as O
    canon, means_at = bouncing_balls(n_per_ball=150, seed=seed)
    W, H = 96, 72
    cam = look_at_camera(W, H, center=(0.4, 0.6, -3.0), target=(0.0, 0.0, 0.0), time=0.3)
    s = dict(canon)
    s.update(means3D=means_at(0.3), bg=np.ones(3, np.float32), sh_degree=3, scale_modifier=1.0, W=W, H=H,
             viewmatrix=cam.world_view_transform.numpy().astype(np.float32),
             projmatrix=cam.full_proj_transform.numpy().astype(np.float32),
             campos=cam.camera_center.numpy().astype(np.float32), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy)
    gt = o_forward(O, s)[1]
    return s, cam, gt


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pose_recovery(seed):
    """Gaussians frozen, one view: the camera starts a twist of 1 degree and 1 % of its distance to the scene away
    from the pose the ground truth was rendered with; after 100 Adam steps on the L1 loss both errors and the loss
    are below their starting values.  The deltas ARE the errors: the refiner perturbs the true camera, so zero
    deltas are the truth."""
    from gs4d_train.pose import PoseRefiner
    from gs4d_train.render import render
    s, cam, gt = _pose_problem(seed)
    dev = torch.device("cuda:0")
    pc = _Canonical(s, dev, requires_grad=False)
    bg = torch.tensor(s["bg"], device=dev)
    gt = torch.tensor(gt, device=dev)
    dist = float(np.linalg.norm(s["campos"]))
    rng = np.random.default_rng(100 + seed)
    axis = rng.normal(size=3)
    tdir = rng.normal(size=3)
    ref = PoseRefiner(1, dev)
    with torch.no_grad():
        ref.rot[0] = torch.tensor(axis / np.linalg.norm(axis) * math.radians(1.0), dtype=torch.float32)
        ref.trans[0] = torch.tensor(tdir / np.linalg.norm(tdir) * 0.01 * dist, dtype=torch.float32)
    r0, t0 = ref.errors()
    # Adam moves a parameter by about lr per step: 1e-3 is 1/17 of the rotation error and 1/30 of the translation
    # error at the start, and 100 steps can cover three times either
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    losses = []
    for _ in range(100):
        pkg = render(cam, pc, False, bg, stage="coarse", camera_grad=True, camera_tensors=ref.tensors(cam))
        loss = (pkg["render"] - gt).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float((render(cam, pc, False, bg, stage="coarse", camera_tensors=ref.tensors(cam))["render"] - gt)
                      .abs().mean())
    r1, t1 = ref.errors()
    print(f"[camera-pose] seed {seed}: rotation {math.degrees(r0):.3f} -> {math.degrees(r1):.3f} deg, translation "
          f"{t0:.4f} -> {t1:.4f}, L1 {losses[0]:.5f} -> {final:.5f}", flush=True)
    assert r1 < r0 and t1 < t0 and final < losses[0]


def test_train_step_with_and_without_a_refiner():
    import test_depth_grad_gpu as TD
    from gs4d_train import config
    from gs4d_train.pose import PoseRefiner
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    W, H, P = 64, 48, 500
    pts, cols = make_point_cloud(P, seed=5)
    views = make_training_views(2, W, H, seed=6)
    for i, (cam, _) in enumerate(views):
        cam.uid = i
    bg = torch.ones(3, device="cuda")
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

    def run(iters, pose_lr=0.0, **kw):
        hyper, opt = config.dynerf()
        opt.pose_lr = pose_lr
        g = TD._train_model(pts, cols, opt, hyper)
        grads = {}
        step = g.optimizer.step

        def recording_step(*a, **k):
            if not grads:
                grads.update({n: getattr(g, n).grad.detach().clone() for n in names})
                grads.update({n: p.grad.detach().clone() for n, p in g._deformation.named_parameters()
                              if p.grad is not None})
            return step(*a, **k)
        g.optimizer.step = recording_step
        losses = [train_step(g, views, opt, hyper, it, bg, **kw).clone() for it in iters]
        params = {n: getattr(g, n).detach().clone() for n in names}
        params.update({n: p.detach().clone() for n, p in g._deformation.named_parameters()})
        return losses, params, grads

    base = run((3001, 3002))
    for kw, lr in ((dict(pose=None), 0.0), (dict(pose=None), 1e-3), (dict(pose=PoseRefiner(2, "cuda")), 0.0)):
        other = run((3001, 3002), pose_lr=lr, **kw)
        assert all(torch.equal(a, b) for a, b in zip(base[0], other[0]))
        assert base[1].keys() == other[1].keys() and all(torch.equal(base[1][n], other[1][n]) for n in base[1])
    ref = PoseRefiner(2, "cuda")
    posed = run((3001, 3002), pose_lr=1e-3, pose=ref)
    assert ref.rot.abs().max() > 0 and ref.trans.abs().max() > 0
    assert torch.isfinite(ref.rot).all() and torch.isfinite(ref.trans).all()
    assert ref.rot.grad is None                                           # stepped and zeroed
    assert torch.equal(posed[0][0], base[0][0])                           # step one: zero deltas, the same forward
    assert base[2].keys() == posed[2].keys() and len(base[2]) > 6
    for n in base[2]:
        assert torch.equal(base[2][n], posed[2][n]), n
    assert not torch.equal(posed[0][1], base[0][1])                       # step two sees the moved cameras
    with pytest.raises(ValueError, match="data_parallel"):
        run((3001,), pose_lr=1e-3, pose=PoseRefiner(2, "cuda"), data_parallel=True)


def test_render_view_takes_camera_tensors():
    import test_infer_gpu as TI
    from gs4d_train import infer
    from gs4d_train.pose import PoseRefiner
    g = TI._shared_model("dnerf")
    cam = TI._cameras(3)[1]
    bg = torch.ones(3, device="cuda")
    state = infer.prepare(g)
    ref = PoseRefiner(1, "cuda")
    plain = infer.render_view(cam, state, bg)
    same = infer.render_view(cam, state, bg, camera_tensors=ref.tensors(cam))
    assert torch.equal(plain["render"], same["render"]) and torch.equal(plain["radii"], same["radii"])
    with torch.no_grad():
        ref.trans[0, 0] = 0.05
    moved = infer.render_view(cam, state, bg, camera_tensors=ref.tensors(cam))
    assert not torch.equal(plain["render"], moved["render"])
