"""Every bound entry point on a side stream and on a second device (tests/stream_cases.py has the harness and the
case table).  The reference of every comparison is the same call on the default stream of device 0, bit for bit:
the operations themselves are pinned against fp64 and the oracle by their own tests.

Each run prints one `[streams]` line with the spin kernel's rate, the delays used and its two conditions (the probe
saw the decoy; the blocker was still running when the side stream had drained)."""
import time

import numpy as np
import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cal():
    return SC.calibration("cuda:0")


_STREAMS = {}


def side_stream(cal, which):
    """the module's side streams, each proven to run alongside the null stream and the earlier ones"""
    if which not in _STREAMS:
        _STREAMS[which] = cal.fresh_stream(apart_from=tuple(_STREAMS.values()))
    return _STREAMS[which]


def run(cal, case, which="first", **kw):
    return SC.run_case(case, side_stream(cal, which), probe_stream=side_stream(cal, "probe"), **kw)


# ---- the harness can fail ------------------------------------------------------------------------------------------
def test_harness_passes_a_correct_operation(cal):
    run(cal, SC.CONTROL_GOOD)
    run(cal, SC.CONTROL_GOOD, blocker=False)


def test_harness_catches_an_early_reader(cal):
    """x * 2 computed on the null stream from inside the side-stream context reads the staging tensor before the
    delayed copies: the decoy's product.  Without the blocker, which would hold that read back until it is right."""
    with pytest.raises(SC.StreamMismatch) as e:
        run(cal, SC.CONTROL_EARLY, blocker=False)
    print(f"[streams] early reader caught: {e.value}", flush=True)


def test_harness_catches_a_late_writer(cal):
    """an output allocated (zeroed) on the side stream and filled on the null stream behind the blocker: the side
    stream's copy to the host reads the zeros"""
    with pytest.raises(SC.StreamMismatch) as e:
        run(cal, SC.CONTROL_LATE)
    print(f"[streams] late writer caught: {e.value}", flush=True)


# ---- the shapes take every launch ----------------------------------------------------------------------------------
def test_raster_scene_fills_several_tiles_and_straddles_waves():
    """the case scene (cam_dense): several tiles, more than 3 x 64 emitted instances, Gaussians whose records straddle
    two waves of the reduction: counted from the forward's own lists"""
    t = SC.to_device(SC.raster_inputs(SC.SEED), "cuda:0")
    fwd = SC.raster_forward(t)
    ranges, order, n, gid, reach, slot, depth = SC.raster_tile_lists(t, fwd)
    P = SC.RASTER["P"]
    gid, slot, ranges = gid.cpu().numpy(), slot.cpu().numpy(), ranges.cpu().numpy()
    first, last = np.full(P, 2 ** 31 - 1, np.int64), np.full(P, -1, np.int64)
    np.minimum.at(first, gid, slot)
    np.maximum.at(last, gid, slot)
    straddling = int(((last >= 0) & (first // 64 != last // 64)).sum())
    tiles = int((ranges[:, 1] > ranges[:, 0]).sum())
    print(f"[streams] raster scene: {n} instances in {tiles} tiles, {straddling} Gaussians straddle two waves", flush=True)
    assert tiles >= 4 and n > 3 * 64 and straddling >= 1


def test_hexplane_points_take_the_window_path_and_the_direct_path():
    import hexplane_path_scenes as HP
    t = SC.to_device(SC.CASES["hexplane_backward"].make(SC.SEED), "cuda:0")
    from gs4d_train import _C
    _, _, order = _C.hexplane_forward(t["pts"], SC._lst(t, "plane_"))
    npw, wcap = HP.plan(SC.HEX_F)
    recs = HP.classify(t["pts"].cpu().numpy(), order.cpu().numpy(), SC.hex_sizes(), SC.HEX_F, npw, wcap)
    classes = {}
    for r in recs:
        classes[r["cls"]] = classes.get(r["cls"], 0) + 1
    print(f"[streams] hexplane case: {npw} points per workgroup, window {wcap} words, classes {classes}", flush=True)
    assert classes.get("direct", 0) >= 1 and classes.get("full", 0) >= 1
    assert len({r["group"] for r in recs}) >= 2


# ---- every entry point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_entry_point_on_a_side_stream(cal, name):
    run(cal, SC.CASES[name])


def test_second_stream_then_the_default_stream(cal):
    """the per-stream scratch and handles then hold more than one key: a second side stream, then stream 0 again"""
    for name in SC.SECOND_STREAM:
        case = SC.CASES[name]
        _, want = run(cal, case, which="second", tag=f"{name} (second stream)")
        again = SC.run_default(case, SC.to_device(case.make(SC.SEED), "cuda:0"))
        d = SC.first_difference(again, want) if case.exact else SC.within_bar(again, want, case.bar)
        assert d is None, f"{name}: the default stream after two side streams: {d}"
        run(cal, case, which="first", tag=f"{name} (first stream again)")


# ---- autograd: the backward runs on the forward's stream -----------------------------------------------------------
_CALLER = {}  # the stream that is current where .backward() is called: neither the forward's nor the blocked null stream


def _autograd_call(t):
    import diff_gaussian_rasterization as dgr
    tx, ty, sm = SC._raster_consts()
    leaf = lambda k: t[k].detach().requires_grad_(True)
    view, proj, campos = leaf("viewmatrix"), leaf("projmatrix"), leaf("campos")
    settings = dgr.GaussianRasterizationSettings(
        image_height=SC.RASTER["H"], image_width=SC.RASTER["W"], tanfovx=tx, tanfovy=ty, bg=t["bg"], scale_modifier=sm,
        viewmatrix=view, projmatrix=proj, sh_degree=SC.RASTER["degree"], campos=campos, prefiltered=False, debug=False)
    means3D, shs, opac, scales, rots = leaf("means3D"), leaf("shs"), leaf("opacities"), leaf("scales"), leaf("rotations")
    means2D = torch.zeros_like(means3D, requires_grad=True)
    rast = dgr.GaussianRasterizer(settings, depth_grad=True, alpha=True, absgrad=True, camera_grad=True)
    color, radii, depth, alpha = rast(means3D=means3D, means2D=means2D, shs=shs, opacities=opac, scales=scales,
                                      rotations=rots)
    loss = (color * t["g_color"]).sum() + (depth * t["g_depth"]).sum() + (alpha * t["g_alpha"]).sum()
    # called outside the forward's stream context, with another stream current: autograd runs each node on its
    # forward's stream, and the glue follows it.  (The other stream is not the null stream: autograd makes the root
    # gradient on the caller's stream and has the forward's stream wait for it, which the blocker would hold up.)
    with torch.cuda.stream(_CALLER["stream"]):
        loss.backward()
    grads = [x.grad for x in (means3D, means2D, shs, opac, scales, rots, view, proj, campos)]
    assert all(g is not None for g in grads) and means2D.absgrad is not None
    return [color.detach(), radii, depth.detach(), alpha.detach(), loss.detach(), *grads, means2D.absgrad]


def test_autograd_backward_follows_the_forward_stream(cal):
    _CALLER["stream"] = side_stream(cal, "second")
    got, want = run(cal, SC.Case("autograd: every rasterizer option", (), SC.raster_inputs, _autograd_call))
    assert len(got) == 15 and float(want[5].abs().max()) > 0 and float(want[14].abs().max()) > 0
    assert float(want[11].abs().max()) > 0 and float(want[12].abs().max()) > 0  # the camera gradients


# ---- a densifying train step ---------------------------------------------------------------------------------------
TRAIN_ITERATIONS = (3001, 3002, 3003, 3004)


def _train_setup():
    from gs4d_train import config
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    hyper, opt = config.dynerf()
    opt.densify_from_iter = 0
    opt.densification_interval = 2        # iterations 3002 and 3004 densify
    opt.densify_grad_threshold_fine_init = opt.densify_grad_threshold_after = 1e-9
    pts, cols = make_point_cloud(2000, seed=5)
    views = make_training_views(2, 96, 64, seed=6)
    return hyper, opt, pts, cols, views


def _train_model(hyper, opt, pts, cols):
    from gs4d_train.gaussians import GaussianModel
    torch.manual_seed(7)
    g = GaussianModel(3, hyper, fused=True)
    g.create_from_pcd(pts, cols, 1.0)
    g._deformation.deformation_net.grid.fused = True
    g._deformation.deformation_net.fused_heads = True
    g.training_setup(opt)
    g.active_sh_degree = 3
    return g


def _train_run(g, hyper, opt, views, before_step=None):
    from gs4d_train.train import train_step
    bg = torch.ones(3, device="cuda")
    losses, counts = [], [g.get_xyz.shape[0]]
    for it in TRAIN_ITERATIONS:
        if before_step is not None:
            before_step()
        losses.append(train_step(g, views, opt, hyper, it, bg))
        counts.append(g.get_xyz.shape[0])
    state = {n: p.detach() for n, p in g._deformation.named_parameters()}
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "xyz_gradient_accum",
                 "denom", "max_radii2D"):
        state[name] = getattr(g, name).detach()
    return torch.stack([l.detach().reshape(()) for l in losses]), counts, state


def test_densifying_train_steps_on_a_side_stream(cal):
    """four fine-stage iterations (two of them densify) of one model under a side stream, the null stream blocked
    for the whole run and a spin queued before each step, against the same model on the default stream afterwards"""
    hyper, opt, pts, cols, views = _train_setup()
    stream, null = side_stream(cal, "first"), torch.cuda.default_stream()
    t_run = 0.0
    for _ in range(2):  # throwaway models: the stream's scratch and handles, the GEMM tuner's choices per point count
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            g = _train_model(hyper, opt, pts, cols)
            stream.synchronize()
            t0 = time.perf_counter()
            _train_run(g, hyper, opt, views)
            stream.synchronize()
            t_run = 1e3 * (time.perf_counter() - t0)
    d_side, _ = SC.delays_ms(cal.enqueue_ms, 0.0)
    d_null = len(TRAIN_ITERATIONS) * d_side + max(SC.FACTOR * t_run, SC.D_NULL_ROOM_MS)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g = _train_model(hyper, opt, pts, cols)
        stream.synchronize()
        with torch.cuda.stream(null):
            cal.spin(d_null)
            ev = torch.cuda.Event()
            ev.record(null)
        losses, counts, state = _train_run(g, hyper, opt, views, before_step=lambda: cal.spin(d_side))
        host = {k: v.cpu() for k, v in state.items()}
        losses = losses.cpu()
        stream.synchronize()
    blocker_running = not ev.query()
    torch.cuda.synchronize()
    print(f"[streams] train steps: P {counts[0]} -> {counts[-1]} ({counts}), four steps {t_run:.1f} ms, D_side "
          f"{d_side:.1f} ms per step, D_null {d_null:.1f} ms, blocker {'running' if blocker_running else 'ENDED'}",
          flush=True)
    assert blocker_running, "blocker too short"
    assert counts[-1] != counts[0], "no iteration densified or pruned"
    ref = _train_model(hyper, opt, pts, cols)
    want_losses, want_counts, want = _train_run(ref, hyper, opt, views)
    torch.cuda.synchronize()
    assert counts == want_counts
    assert SC.first_difference([losses], [want_losses]) is None, (losses, want_losses)
    assert set(host) == set(want) and any("grid" in k for k in want)
    differ = [k for k in want if SC.first_difference([host[k]], [want[k]]) is not None]
    assert not differ, differ


# ---- a second device -----------------------------------------------------------------------------------------------
two_devices = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU (one device visible)")


@two_devices
@pytest.mark.parametrize("name", SC.SECOND_DEVICE)
def test_tensors_on_the_second_device(name):
    """device 0 current, no device context: the outputs live on cuda:1 and hold device 0's bytes"""
    case = SC.CASES[name]
    assert torch.cuda.current_device() == 0
    want = SC.run_default(case, SC.to_device(case.make(SC.SEED), "cuda:0"))
    got = [o.detach() for o in case.call(SC.to_device(case.make(SC.SEED), "cuda:1"))]
    assert torch.cuda.current_device() == 0
    assert all(o.device == torch.device("cuda:1") for o in got)
    torch.cuda.synchronize("cuda:1")
    d = SC.first_difference(got, want) if case.exact else SC.within_bar(got, want, case.bar)
    assert d is None, f"{name} on cuda:1: {d}"


@two_devices
@pytest.mark.parametrize("name", SC.SECOND_DEVICE)
def test_side_stream_of_the_second_device(name):
    cal1 = SC.calibration("cuda:1")
    if "cuda:1" not in _STREAMS:
        _STREAMS["cuda:1"] = cal1.fresh_stream()
        _STREAMS["cuda:1 probe"] = cal1.fresh_stream(apart_from=(_STREAMS["cuda:1"],))
    case = SC.CASES[name]
    got, _ = SC.run_case(case, _STREAMS["cuda:1"], probe_stream=_STREAMS["cuda:1 probe"], tag=f"{name} (cuda:1)")
    want = SC.run_default(case, SC.to_device(case.make(SC.SEED), "cuda:0"))
    d = SC.first_difference(got, want) if case.exact else SC.within_bar(got, want, case.bar)
    assert d is None, f"{name} on a side stream of cuda:1 against device 0: {d}"
    assert torch.cuda.current_device() == 0


@two_devices
def test_forwards_alternate_between_two_devices():
    """one thread, the forward's pinned readback word and event per device"""
    case = SC.CASES["rasterize_gaussians[sh]"]
    ins = {d: [SC.to_device(case.make(SC.SEED + k), d) for k in (0, 1)] for d in ("cuda:0", "cuda:1")}
    want = [SC.run_default(case, ins["cuda:0"][k]) for k in (0, 1)]
    for k in (0, 1, 0, 1):
        for d in ("cuda:0", "cuda:1"):
            got = case.call(ins[d][k])
            assert SC.first_difference(got, want[k]) is None, (d, k)
