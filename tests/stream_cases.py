"""Every bound entry point on a side stream: the case table and the harness (tests/test_streams_boundary.py,
tests/test_streams_gpu.py).

The operations are pinned against fp64 and the oracle elsewhere; nothing here is a numerical reference.  The
reference of a case is the same call on the default stream, and the comparison is bitwise.

The harness (run_case) forces the two races a stream bug allows.  A spin kernel (the blocker) holds the null
stream for the whole side-stream run, so a launch, memset or copy that went to the null stream instead of the
caller's runs after its consumers and after the result was read.  The inputs reach the staging tensors through
copies queued on the side stream behind a second spin, so work that reads them on any other stream sees the decoy
(another valid input set of the same shapes) that the staging tensors held before.  Two assertions per run are the
conditions: a clone of a staged tensor taken on a third stream still shows the decoy (the copies had not run when
the call was queued), and the blocker's event has not completed when the side stream has drained.

A case: make(seed) -> an ordered dict of CPU tensors (the inputs; everything the call reads from the device),
call(t) -> the list of output tensors, on whatever stream is current, for t the same dict on a device.  In-place
entries return the tensors they wrote.
"""
import collections
import math
import os
import re
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dgaussians-fast-train_amd", "csrc")
GLUE = ("torch_glue.cpp", "train_glue.cpp", "knn_glue.cpp")
SEED = 1  # real = make(SEED), decoy = make(SEED + 1); the rasterizer's real scene is camera_grad_refs' cam_dense


def bound_names():
    """every name an extension module binds: m.def("name" or m.def(\\n "name" in the three glue files"""
    names = []
    for f in GLUE:
        with open(os.path.join(CSRC, f)) as fh:
            names += re.findall(r'm\.def\(\s*"(\w+)"', fh.read())
    return names


# ---- comparison -----------------------------------------------------------------------------------------------------
class StreamMismatch(AssertionError):
    """the side-stream bytes differ from the default stream's"""


class HarnessInvalid(AssertionError):
    """a run whose races were not forced (the probe saw the real input, or the blocker ended early)"""


def bits(t):
    """the tensor's bytes as integers of its element size (so -0.0 != +0.0 and equal NaN bits are equal)"""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if t.is_floating_point():
        t = t.contiguous()
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def first_difference(got, want):
    """None when the two lists of tensors agree in length, shapes, dtypes and every bit; else a description"""
    if len(got) != len(want):
        return f"{len(got)} outputs against {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
            return f"output {i}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
        ba, bb = bits(a.cpu()), bits(b.cpu())
        if not torch.equal(ba, bb):
            bad = (ba != bb).reshape(-1)
            k = int(torch.nonzero(bad)[0])
            return (f"output {i}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {k}: "
                    f"{a.cpu().reshape(-1)[k].item()!r} against {b.cpu().reshape(-1)[k].item()!r}")
    return None


def within_bar(got, want, rel):
    """exact=False cases: every output within rel of the reference's largest magnitude (the operation's own test's
    bar, cited at the case)"""
    if len(got) != len(want):
        return f"{len(got)} outputs against {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
            return f"output {i}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
        a, b = a.cpu().double(), b.cpu().double()
        err, scale = float((a - b).abs().max()) if a.numel() else 0.0, float(b.abs().max()) if b.numel() else 0.0
        if not err <= rel * scale:
            return f"output {i}: off by {err:.3e}, bar {rel * scale:.3e}"
    return None


# ---- delays ---------------------------------------------------------------------------------------------------------
D_SIDE_FLOOR_MS = 5.0    # the side stream's spin is never shorter: a clone on another stream takes microseconds
D_NULL_ROOM_MS = 20.0    # the blocker outlasts the side spin by at least this much
FACTOR = 10.0


def delays_ms(enqueue_ms, t_case_ms):
    """(D_side, D_null) from the largest host enqueue time seen and the case's wall time (enqueue + synchronise):
    D_side >= 10 x the enqueue time, D_null >= D_side + 10 x t_case.  The factors only give the run's two assertions
    room; the assertions are the conditions."""
    if not (enqueue_ms >= 0 and t_case_ms >= 0 and math.isfinite(enqueue_ms) and math.isfinite(t_case_ms)):
        raise ValueError("delays_ms: measurements must be finite and non-negative")
    d_side = max(FACTOR * enqueue_ms, D_SIDE_FLOOR_MS)
    d_null = d_side + max(FACTOR * t_case_ms, D_NULL_ROOM_MS)
    return d_side, d_null


def cycles_for(ms, cycles_per_ms):
    if not cycles_per_ms > 0:
        raise ValueError("cycles_for: the spin kernel's rate must be positive")
    return max(1, int(math.ceil(ms * cycles_per_ms)))


class Calibration:
    """the spin kernel's cycles per millisecond on one device, and the session's running maxima"""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cycles_per_ms = None
        self.enqueue_ms = 0.0     # largest host enqueue time of a case's call seen so far
        self.t_case_ms = 0.0      # largest case wall time seen so far
        self.d_side_ms = self.d_null_ms = 0.0  # largest delays used
        self._streams = {}

    def measure(self):
        if self.cycles_per_ms is None:
            with torch.cuda.device(self.device):
                s = torch.cuda.default_stream(self.device)
                rate = None
                for n in (1_000_000, 20_000_000):  # the first spin also loads the kernel
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    torch.cuda._sleep(n)
                    e1.record(s)
                    e1.synchronize()
                    rate = n / max(e0.elapsed_time(e1), 1e-6)
                self.cycles_per_ms = rate
        return self.cycles_per_ms

    def spin(self, ms):
        """a spin of `ms` on the current stream"""
        torch.cuda._sleep(cycles_for(ms, self.measure()))

    def concurrent(self, stream, busy):
        """whether `stream` runs while `busy` spins (two streams may share a hardware queue, which orders them)"""
        with torch.cuda.stream(busy):
            self.spin(D_SIDE_FLOOR_MS)
            ev = torch.cuda.Event()
            ev.record(busy)
        with torch.cuda.stream(stream):
            x = torch.zeros(16, device=self.device) + 1
        stream.synchronize()
        ok = not ev.query()
        torch.cuda.synchronize(self.device)
        return ok

    def fresh_stream(self, apart_from=()):
        """a new torch.cuda.Stream that runs alongside the null stream and every stream of `apart_from`"""
        null = torch.cuda.default_stream(self.device)
        tried = 0
        while tried < 64:
            tried += 1
            s = torch.cuda.Stream(device=self.device)
            if s in apart_from or s == null:
                continue
            if all(self.concurrent(s, b) for b in (null, *apart_from)):
                return s
        raise HarnessInvalid("no stream runs alongside the null stream: every candidate shares its queue")


_CAL = {}


def calibration(device="cuda:0"):
    device = torch.device(device)
    if device not in _CAL:
        _CAL[device] = Calibration(device)
        _CAL[device].measure()
    return _CAL[device]


# ---- the harness ----------------------------------------------------------------------------------------------------
def to_device(t, device):
    return collections.OrderedDict((k, v.to(device).clone()) for k, v in t.items())


def clone_inputs(t):
    return collections.OrderedDict((k, v.clone()) for k, v in t.items())


def probe_key(real, decoy):
    """the first input whose bytes differ between the two sets"""
    for k in real:
        if real[k].numel() and not torch.equal(bits(real[k]), bits(decoy[k])):
            return k
    raise HarnessInvalid("the decoy equals the real input")


def run_default(case, real):
    """the reference: the call on the device's default stream, from a private copy of the inputs"""
    return [o.detach().clone() for o in case.call(clone_inputs(real))]


def run_case(case, stream, seed=SEED, blocker=True, probe_stream=None, tag=None):
    """the case on `stream` under the forced races, against the same call on the default stream afterwards.
    Raises StreamMismatch when the bytes differ and HarnessInvalid when a race was not forced.  blocker=False: no spin
    on the null stream (the early-reader control, whose fault is work on the null stream that must run early)."""
    dev = stream.device
    cal = calibration(dev)
    null = torch.cuda.default_stream(dev)
    with torch.cuda.device(dev):
        if probe_stream is None:
            probe_stream = cal.fresh_stream(apart_from=(stream,))
        real, decoy = to_device(case.make(seed), dev), to_device(case.make(seed + 1), dev)
        key = probe_key(real, decoy)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            # warm-up on the decoy: the stream's scratch, handles and allocator blocks; then once more, timed
            staged = clone_inputs(decoy)
            case.call(staged)
            stream.synchronize()
            for k in staged:
                staged[k].copy_(decoy[k])
            stream.synchronize()
            t0 = time.perf_counter()
            warm = case.call(staged)
            t1 = time.perf_counter()
            stream.synchronize()
            t2 = time.perf_counter()
            for k in staged:
                staged[k].copy_(decoy[k])
            host = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in warm]
            del warm
            stream.synchronize()
        with torch.cuda.stream(probe_stream):
            probe = staged[key].clone()   # its block, for the real probe below
            probe_stream.synchronize()
        cal.enqueue_ms = max(cal.enqueue_ms, 1e3 * (t1 - t0))
        t_case = 1e3 * (t2 - t0)
        cal.t_case_ms = max(cal.t_case_ms, t_case)
        d_side, d_null = delays_ms(cal.enqueue_ms, t_case)
        cal.d_side_ms, cal.d_null_ms = max(cal.d_side_ms, d_side), max(cal.d_null_ms, d_null)
        ev = None
        if blocker:
            with torch.cuda.stream(null):
                cal.spin(d_null)
                ev = torch.cuda.Event()
                ev.record(null)
        with torch.cuda.stream(stream):
            cal.spin(d_side)
            for k in staged:
                staged[k].copy_(real[k], non_blocking=True)
        with torch.cuda.stream(probe_stream):
            probe.copy_(staged[key], non_blocking=True)
        with torch.cuda.stream(stream):
            got = case.call(staged)
            same_shapes = len(got) == len(host) and all(tuple(o.shape) == tuple(h.shape) and o.dtype == h.dtype
                                                        for o, h in zip(got, host))
            if same_shapes:
                for h, o in zip(host, got):
                    h.copy_(o, non_blocking=True)
            else:  # the outputs' sizes follow the data (another point count): pageable copies on this stream
                host = [o.cpu() for o in got]
            stream.synchronize()
        blocker_running = ev is None or not ev.query()
        torch.cuda.synchronize(dev)
        probe_saw_decoy = torch.equal(bits(probe), bits(decoy[key]))
        print(f"[streams] {tag or case.name}: {cal.cycles_per_ms:.0f} cycles/ms, enqueue max {cal.enqueue_ms:.3f} ms, "
              f"t_case {t_case:.3f} ms, D_side {d_side:.1f} ms, D_null {d_null if blocker else 0.0:.1f} ms, probe "
              f"{'decoy' if probe_saw_decoy else 'REAL'}, blocker {'running' if blocker_running else 'ENDED'}",
              flush=True)
        if not probe_saw_decoy:
            raise HarnessInvalid(f"{case.name}: the probe saw the real input (the side delay is too short)")
        if not blocker_running:
            raise HarnessInvalid(f"{case.name}: blocker too short")
        want = run_default(case, real)
        if case.exact:
            again = run_default(case, real)
            d = first_difference(again, want)
            if d is not None:
                raise AssertionError(f"{case.name}: two default-stream runs differ: {d}")
            d = first_difference(host, want)
        else:
            d = within_bar(host, want, case.bar)
        torch.cuda.synchronize(dev)
        if d is not None:
            raise StreamMismatch(f"{case.name} on {stream}: {d}")
        return host, want


# ---- the case table -------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, entries, make, call, exact=True, bar=None):
        self.name, self.entries, self.make, self.call, self.exact, self.bar = name, tuple(entries), make, call, exact, bar

    def __repr__(self):
        return f"Case({self.name})"


CASES = collections.OrderedDict()


def case(name, entries, make, exact=True, bar=None):
    def deco(call):
        assert name not in CASES
        CASES[name] = Case(name, entries, make, call, exact, bar)
        return call
    return deco


def _g(seed):
    return torch.Generator().manual_seed(int(seed))


def _od(**kw):
    return collections.OrderedDict(kw)


def _R():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def _T():
    from gs4d_train import _C
    return _C


# ---- rasterizer: camera_grad_refs' cam_dense (depth_scenes._dense: 300 Gaussians, 40 x 24, six tiles) ---------------
RASTER = dict(P=300, W=40, H=24, degree=3)
_RASTER_CACHE = {}


def raster_scene(seed):
    """depth_scenes._dense(seed): seed 1 is cam_dense itself"""
    if seed not in _RASTER_CACHE:
        import depth_scenes as DS
        s = DS._dense(seed)
        assert s["means3D"].shape[0] == RASTER["P"] and (s["W"], s["H"]) == (RASTER["W"], RASTER["H"])
        _RASTER_CACHE[seed] = s
    return _RASTER_CACHE[seed]


def raster_inputs(seed):
    s = raster_scene(seed)
    rng = np.random.default_rng(seed + 100)
    P, H, W = RASTER["P"], RASTER["H"], RASTER["W"]
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32))
    return _od(means3D=f(s["means3D"]), opacities=f(s["opacities"]), scales=f(s["scales"]), rotations=f(s["rotations"]),
               shs=f(s["shs"]), colors=f(rng.uniform(0, 1, (P, 3))), bg=f(rng.uniform(0, 1, 3)),
               viewmatrix=f(s["viewmatrix"]), projmatrix=f(s["projmatrix"]), campos=f(s["campos"]),
               g_color=f(rng.normal(0, 1, (3, H, W))), g_depth=f(rng.normal(0, 1, (1, H, W))),
               g_alpha=f(rng.normal(0, 1, (1, H, W))))


def _raster_consts():
    s = raster_scene(SEED)
    return float(s["tanfovx"]), float(s["tanfovy"]), float(s["scale_modifier"])


def raster_forward(t, colors=False, aa=None):
    """(num_rendered, color, depth, radii, geometry, binning, image states)"""
    tx, ty, sm = _raster_consts()
    e = torch.empty(0, device=t["means3D"].device)
    args = (t["bg"], t["means3D"], t["colors"] if colors else e, t["opacities"], t["scales"], t["rotations"], sm, e,
            t["viewmatrix"], t["projmatrix"], tx, ty, RASTER["H"], RASTER["W"], e if colors else t["shs"],
            RASTER["degree"], t["campos"], False, False)
    if aa is None:
        return _R().rasterize_gaussians(*args)
    return _R().rasterize_gaussians_aa(*args, aa)


def _fwd_outputs(fwd, like):
    return [torch.tensor([fwd[0]], dtype=torch.int32, device=like.device), fwd[1], fwd[2], fwd[3]]


def raster_backward(t, fwd, entry, images, tail=(), colors=False):
    tx, ty, sm = _raster_consts()
    e = torch.empty(0, device=t["means3D"].device)
    nr, color, depth, radii, gb, bb, ib = fwd
    args = (t["bg"], t["means3D"], radii, t["colors"] if colors else e, t["scales"], t["rotations"], sm, e,
            t["viewmatrix"], t["projmatrix"], tx, ty, *images, e if colors else t["shs"], RASTER["degree"], t["campos"],
            gb, nr, bb, ib, False, *tail)
    return list(getattr(_R(), entry)(*args))


@case("rasterize_gaussians[sh]", ["rasterize_gaussians"], raster_inputs)
def _(t):
    return _fwd_outputs(raster_forward(t), t["means3D"])


@case("rasterize_gaussians[colors_precomp]", ["rasterize_gaussians"], raster_inputs)
def _(t):
    return _fwd_outputs(raster_forward(t, colors=True), t["means3D"])


@case("rasterize_gaussians_aa", ["rasterize_gaussians_aa"], raster_inputs)
def _(t):
    return _fwd_outputs(raster_forward(t, aa=True), t["means3D"])


# the backward entries: the forward runs inside the same call, so its host readback sits in the middle
@case("rasterize_gaussians_backward", ["rasterize_gaussians_backward"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    return raster_backward(t, fwd, "rasterize_gaussians_backward", (t["g_color"],))


@case("rasterize_gaussians_backward[colors_precomp]", ["rasterize_gaussians_backward"], raster_inputs)
def _(t):
    fwd = raster_forward(t, colors=True)
    return raster_backward(t, fwd, "rasterize_gaussians_backward", (t["g_color"],), colors=True)


@case("rasterize_gaussians_backward_depth", ["rasterize_gaussians_backward_depth"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    return raster_backward(t, fwd, "rasterize_gaussians_backward_depth", (t["g_color"], t["g_depth"]))


@case("rasterize_gaussians_backward_aux", ["rasterize_gaussians_backward_aux"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    return raster_backward(t, fwd, "rasterize_gaussians_backward_aux", (t["g_color"], t["g_depth"], t["g_alpha"]))


@case("rasterize_gaussians_backward_absgrad", ["rasterize_gaussians_backward_absgrad"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    return raster_backward(t, fwd, "rasterize_gaussians_backward_absgrad", (t["g_color"], t["g_depth"], t["g_alpha"]))


@case("rasterize_gaussians_backward_aa", ["rasterize_gaussians_backward_aa"], raster_inputs)
def _(t):
    fwd = raster_forward(t, aa=True)
    return raster_backward(t, fwd, "rasterize_gaussians_backward_aa", (t["g_color"], t["g_depth"], t["g_alpha"]),
                           tail=(t["opacities"], True, True))


@case("rasterize_gaussians_backward_camera", ["rasterize_gaussians_backward_camera"], raster_inputs)
def _(t):
    fwd = raster_forward(t, aa=True)
    return raster_backward(t, fwd, "rasterize_gaussians_backward_camera", (t["g_color"], t["g_depth"], t["g_alpha"]),
                           tail=(t["opacities"], True, True))


@case("alpha_image", ["alpha_image"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    return [_R().alpha_image(fwd[6], RASTER["H"], RASTER["W"])]


@case("mark_visible", ["mark_visible"], raster_inputs)
def _(t):
    return [_R().mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"])]


def raster_tile_lists(t, fwd):
    out = _R().debug_tile_lists(fwd[4], fwd[5], fwd[6], RASTER["P"], RASTER["W"], RASTER["H"], fwd[0])
    return out  # (ranges, order, L', gid, reach, slot, depth)


@case("debug_tile_lists", ["debug_tile_lists"], raster_inputs)
def _(t):
    out = raster_tile_lists(t, raster_forward(t))
    return [out[0], out[1], torch.tensor([out[2]], dtype=torch.int32, device=out[0].device), *out[3:]]


@case("debug_effective_opacity", ["debug_effective_opacity"], raster_inputs)
def _(t):
    fwd = raster_forward(t, aa=True)
    o = _R().debug_effective_opacity(fwd[4], RASTER["P"])
    return [torch.where(fwd[3] > 0, o, torch.zeros_like(o))]  # a culled Gaussian's record is not written


@case("debug_pair_alpha", ["debug_pair_alpha"], raster_inputs)
def _(t):
    fwd = raster_forward(t)
    lists = raster_tile_lists(t, fwd)
    n = min(int(lists[2]), 256)
    gid = lists[3][:n].contiguous()  # Gaussians that reach a pixel: their records are written
    k = torch.arange(n, device=gid.device, dtype=torch.int32)
    og, pw = _R().debug_pair_alpha(fwd[4], RASTER["P"], RASTER["W"], RASTER["H"], gid, (7 * k) % RASTER["W"],
                                   (5 * k) % RASTER["H"])
    return [gid, og, pw]


def _wave_inputs(seed):
    return _od(x=torch.randn(5, 20, 64, generator=_g(seed)))


@case("debug_wave_sum", ["debug_wave_sum"], _wave_inputs)
def _(t):
    out = []
    for depth, absg in ((False, False), (True, False), (False, True), (True, True)):
        out += list(_R().debug_wave_sum(t["x"], depth, absg))
    return out


# ---- simple_knn ------------------------------------------------------------------------------------------------------
def _knn_inputs(seed):
    """test_gpu_edge_sizes' largest cloud: 4097 normal points"""
    return _od(x=torch.tensor(np.random.default_rng(seed + 11).normal(size=(4097, 3)).astype(np.float32)))


@case("distCUDA2", ["distCUDA2"], _knn_inputs)
def _(t):
    from simple_knn._C import distCUDA2
    return [distCUDA2(t["x"])]


# ---- losses and statistics --------------------------------------------------------------------------------------------
def _l1_inputs(n):
    def make(seed):
        import train_edge_refs as TR
        x, y = TR.l1_inputs(n, seed=seed)
        return _od(x=x.clone(), y=y.clone(), dloss=torch.rand(1, generator=_g(seed)) + 0.5)
    return make


L1_N = 17 * 2048 + 4  # several workgroups, a ragged last one, numel % 4 == 0 (l1_loss_grad's float4 form)


@case("l1_forward", ["l1_forward"], _l1_inputs(L1_N + 1))
def _(t):
    return list(_T().l1_forward(t["x"], t["y"]))


@case("l1_backward", ["l1_backward"], _l1_inputs(L1_N + 1))
def _(t):
    loss, sign = _T().l1_forward(t["x"], t["y"])
    return [_T().l1_backward(sign, t["dloss"])]


@case("l1_loss_grad", ["l1_loss_grad"], _l1_inputs(L1_N))
def _(t):
    return list(_T().l1_loss_grad(t["x"], t["y"], 0.37))


def _aux_inputs(seed):
    g = _g(seed)
    H, W = 45, 70
    gt_d = torch.rand(1, H, W, generator=g) * 4
    gt_d[0, ::5, ::3] = 0.0  # pixels without a depth
    return _od(depth=torch.rand(1, H, W, generator=g) * 4, alpha=torch.rand(1, H, W, generator=g), gt_depth=gt_d,
               gt_mask=(torch.rand(1, H, W, generator=g) > 0.5).float())


@case("aux_loss_grad", ["aux_loss_grad"], _aux_inputs)
def _(t):
    T = _T()
    e = torch.empty(0, device=t["depth"].device)
    both = T.aux_loss_grad(t["depth"], t["alpha"], t["gt_depth"], t["gt_mask"], 0.3, 0.7)
    mask = T.aux_loss_grad(e, t["alpha"], e, t["gt_mask"], 0.0, 0.7)
    return [*both, mask[0], mask[2]]


def _ssim_inputs(seed):
    g = _g(seed)
    x = torch.rand(2, 3, 45, 70, generator=g)
    return _od(x=x, y=(x + 0.2 * torch.randn(2, 3, 45, 70, generator=g)).clamp(0, 1), dvalue=torch.randn(2, generator=g))


@case("ssim_forward", ["ssim_forward"], _ssim_inputs)
def _(t):
    mean, per, maps = _T().ssim_forward(t["x"], t["y"], True)
    mean2, per2, _ = _T().ssim_forward(t["x"], t["y"], False)
    return [mean, per, maps, mean2, per2]


@case("ssim_backward", ["ssim_backward"], _ssim_inputs)
def _(t):
    _, _, maps = _T().ssim_forward(t["x"], t["y"], True)
    return [_T().ssim_backward(t["x"], t["y"], maps, t["dvalue"]),
            _T().ssim_backward(t["x"], t["y"], maps, t["dvalue"][:1].reshape(()))]


@case("l1_dssim_loss_grad", ["l1_dssim_loss_grad"], _ssim_inputs)
def _(t):
    return list(_T().l1_dssim_loss_grad(t["x"], t["y"], 0.2, 0.5))


def _densify_inputs(seed):
    import train_edge_refs as TR
    vs4, vis, radii, acc, den, mr = TR.densify_inputs(1027, seed=seed)
    return _od(vs=vs4[:, :3].contiguous(), vis=vis, radii=radii, acc=acc, den=den, mr=mr,
               acc2=acc.clone() + 1, den2=den.clone(), mr2=mr.clone())


@case("densify_stats", ["densify_stats"], _densify_inputs)
def _(t):
    T = _T()
    T.densify_stats(t["vs"], t["vis"], t["radii"], t["acc"], t["den"], t["mr"])
    T.densify_stats(t["vs"], torch.empty(0, dtype=torch.bool, device=t["vs"].device), t["radii"], t["acc2"], t["den2"],
                    t["mr2"])  # the mask radii > 0 formed inside the kernel
    return [t["acc"], t["den"], t["mr"], t["acc2"], t["den2"], t["mr2"]]


ADAM_SHAPES = ((4096,), (10, 13), (4099,))  # float4 body alone; numel % 4 == 2; a body and a tail of 3


def _adam_inputs(seed):
    g = _g(seed)
    out = collections.OrderedDict()
    for i, sh in enumerate(ADAM_SHAPES):
        out[f"p{i}"] = torch.randn(*sh, generator=g)
        out[f"g{i}"] = torch.randn(*sh, generator=g) * (1e-3, 1.0, 1e3)[i]
        out[f"m{i}"] = torch.randn(*sh, generator=g) * 0.1
        out[f"v{i}"] = torch.rand(*sh, generator=g) * 0.01
    return out


@case("adam_step", ["adam_step"], _adam_inputs)
def _(t):
    import train_edge_refs as TR
    n = len(ADAM_SHAPES)
    col = lambda c: [t[f"{c}{i}"] for i in range(n)]
    ss, bs = zip(*[TR.adam_scalars(TR.ADAM_LR * (i + 1), 0.9, 0.999, 3 + i) for i in range(n)])
    _T().adam_step(col("p"), col("g"), col("m"), col("v"), list(ss), list(bs), 0.9, 0.999, 1e-15)
    return col("p") + col("m") + col("v")


# ---- deformation tail and surgery -------------------------------------------------------------------------------------
TAIL_P, TAIL_K = 777, 16
_TAIL_NAMES = ("xyz", "s", "r", "o", "f_dc", "f_rest", "dx", "ds", "dr", "do", "dshs", "g_means", "g_scales", "g_rot",
               "g_opac", "g_shs")


def _tail_inputs(seed):
    import train_edge_refs as TR
    base, deltas, ups = TR.deform_inputs(TAIL_P, TAIL_K, "all", seed=seed)
    return collections.OrderedDict(zip(_TAIL_NAMES, [x.clone() for x in base + deltas + ups]))


def _tail_forward(t, mixed=False):
    d = [t["dx"], None if mixed else t["ds"], t["dr"], None if mixed else t["do"], t["dshs"]]
    return _T().deform_tail_forward(t["xyz"], t["s"], t["r"], t["o"], t["f_dc"], t["f_rest"], *d)


@case("deform_tail_forward", ["deform_tail_forward"], _tail_inputs)
def _(t):
    return list(_tail_forward(t)) + list(_tail_forward(t, mixed=True))


@case("deform_tail_backward", ["deform_tail_backward"], _tail_inputs)
def _(t):
    means, scales, rot, opac, shs = _tail_forward(t)
    out = _T().deform_tail_backward(scales, t["r"], t["dr"], opac, t["g_means"], t["g_scales"], t["g_rot"], t["g_opac"],
                                    t["g_shs"].reshape(TAIL_P, 3 * TAIL_K), TAIL_K, [True, True, True, True])
    return [o for o in out if o is not None]


ROWS_P, ROWS_A = 1000, 300


def _rows_inputs(seed):
    g = _g(seed)
    P, A = ROWS_P, ROWS_A
    keep = torch.nonzero(torch.rand(P, generator=g) > 0.25).reshape(-1).to(torch.int32)
    keep = torch.cat([keep, torch.zeros(P, dtype=torch.int32)])[:700].contiguous()  # K = 700 whatever the draw
    return _od(xyz=torch.randn(P, 3, generator=g), rest=torch.randn(P, 15, 3, generator=g),
               flag=(torch.rand(P, generator=g) > 0.5).to(torch.uint8), acc=torch.rand(P, 1, generator=g),
               mom=torch.randn(P, 3, generator=g), keep=keep,
               append=torch.randint(0, P, (A,), generator=g, dtype=torch.int32),
               given=torch.randn(100, 3, generator=g))


@case("rows_assemble", ["rows_assemble"], _rows_inputs)
def _(t):
    # GATHER with given rows, GATHER without, GATHER of bytes, ZERO (statistics), ZERO_NEW (optimizer moments)
    return list(_T().rows_assemble([t["xyz"], t["rest"], t["flag"], t["acc"], t["mom"]],
                                   [t["given"], None, None, None, None], [0, 0, 0, 2, 1], t["keep"], t["append"], ROWS_A))


def _slices_inputs(S):
    return lambda seed: _od(parts=torch.randn(S, 129, 65, generator=_g(seed)))


@case("sum_slices[5]", ["sum_slices"], _slices_inputs(5))
def _(t):
    return [_T().sum_slices(t["parts"])]


@case("sum_slices[16]", ["sum_slices"], _slices_inputs(16))
def _(t):
    return [_T().sum_slices(t["parts"])]


# ---- the deformation MLP ----------------------------------------------------------------------------------------------
def _heads_inputs(P, W, ns):
    """test_heads_block_forward_matches_fp64's operands"""
    def make(seed):
        g = _g(seed)
        k = len(ns)
        out = _od(h=torch.relu(torch.randn(P, W, generator=g)), w1=torch.randn(k * W, W, generator=g) / W ** 0.5,
                  b1=torch.randn(k * W, generator=g) * 0.1, a=torch.relu(torch.randn(P, k * W, generator=g)))
        for i, n in enumerate(ns):
            out[f"w2_{i}"] = torch.randn(n, W, generator=g) / W ** 0.5
            out[f"b2_{i}"] = torch.randn(n, generator=g)
            out[f"g_{i}"] = torch.randn(P, n, generator=g)
        return out
    return make


def _lst(t, prefix):
    return [t[k] for k in t if k.startswith(prefix)]


HEADS_SMALL = (777, 64, (2, 16, 5))
HEADS_WIDE = (300, 128, (3, 3, 4, 1, 48))  # the 48-wide head: the MFMA kernels of the backward


@case("linear_dw", ["linear_dw"], _heads_inputs(*HEADS_SMALL))
def _(t):
    W = HEADS_SMALL[1]
    xs = [t["a"][:, i * W:(i + 1) * W] for i in range(len(HEADS_SMALL[2]))]  # row strides kept, as the train step's
    return list(_T().linear_dw(_lst(t, "g_"), xs))


for _name, _shape in (("777x64", HEADS_SMALL), ("300x128", HEADS_WIDE)):
    @case(f"heads_forward[{_name}]", ["heads_forward"], _heads_inputs(*_shape))
    def _(t):
        return list(_T().heads_forward(t["a"], _lst(t, "w2_"), _lst(t, "b2_")))

    @case(f"heads_block_forward[{_name}]", ["heads_block_forward"], _heads_inputs(*_shape))
    def _(t):
        return list(_T().heads_block_forward(t["h"], t["w1"], t["b1"], _lst(t, "w2_"), _lst(t, "b2_")))

    @case(f"heads_block_forward_bf16[{_name}]", ["heads_block_forward_bf16"], _heads_inputs(*_shape))
    def _(t):
        T = _T()
        out = list(T.heads_block_forward_bf16(t["h"], t["w1"], t["b1"], _lst(t, "w2_"), _lst(t, "b2_")))
        again = T.heads_block_forward_bf16(t["h"], t["w1"], t["b1"], _lst(t, "w2_"), _lst(t, "b2_"), hb=out[1])
        return out + [again[0]] + list(again[2:])

    @case(f"heads_backward[f32 {_name}]", ["heads_backward"], _heads_inputs(*_shape))
    def _(t):
        return list(_T().heads_backward(t["a"], _lst(t, "g_"), _lst(t, "w2_")))

    @case(f"heads_backward[bf16 {_name}]", ["heads_backward"], _heads_inputs(*_shape))
    def _(t):
        return list(_T().heads_backward(t["a"].to(torch.bfloat16), _lst(t, "g_"), _lst(t, "w2_")))


def _gemm_inputs(P, KW, W):
    """test_mlp_f32_gemms_match_fp64's operands"""
    def make(seed):
        g = _g(seed)
        w1 = torch.randn(KW, W, generator=g) / KW ** 0.5
        return _od(da=torch.randn(P, KW, generator=g), h=torch.relu(torch.randn(P, W, generator=g)),
                   w1t=w1.t().contiguous())
    return make


for _P, _KW, _W in ((777, 192, 64), (300, 640, 128)):
    @case(f"mlp_dx_f32[{_P}x{_KW}x{_W}]", ["mlp_dx_f32"], _gemm_inputs(_P, _KW, _W))
    def _(t):
        return [_T().mlp_dx_f32(t["da"], t["w1t"])]

    @case(f"mlp_dw_f32[{_P}x{_KW}x{_W}]", ["mlp_dw_f32"], _gemm_inputs(_P, _KW, _W))
    def _(t):
        return [_T().mlp_dw_f32(t["da"], t["h"])]

    @case(f"mlp_dx_bf16[{_P}x{_KW}x{_W}]", ["mlp_dx_bf16"], _gemm_inputs(_P, _KW, _W))
    def _(t):
        return [_T().mlp_dx_bf16(t["da"].to(torch.bfloat16), t["w1t"].to(torch.bfloat16))]

for _P, _KW in ((777, 256), (300, 640)):  # the bf16 weight gradient is built for W = 128
    @case(f"mlp_dw_bf16[{_P}x{_KW}x128]", ["mlp_dw_bf16"], _gemm_inputs(_P, _KW, 128))
    def _(t):
        return [_T().mlp_dw_bf16(t["da"].to(torch.bfloat16), t["h"].to(torch.bfloat16))]


def _feature_inputs(P, Fin, Fout):
    """test_feature_relu_backward_matches_fp64's operands"""
    def make(seed):
        g = _g(seed)
        return _od(x=torch.randn(P, Fin, generator=g), w=torch.randn(Fout, Fin, generator=g) / Fin ** 0.5,
                   b=torch.randn(Fout, generator=g) * 0.1, g=torch.randn(P, Fout, generator=g))
    return make


for _P, _Fin, _Fout in ((777, 64, 64), (300, 32, 128)):
    @case(f"feature_relu_forward[{_P}x{_Fin}x{_Fout}]", ["feature_relu_forward"], _feature_inputs(_P, _Fin, _Fout))
    def _(t):
        return list(_T().feature_relu_forward(t["x"], t["w"], t["b"]))

    @case(f"feature_relu_forward[with_hb {_P}x{_Fin}x{_Fout}]", ["feature_relu_forward"],
          _feature_inputs(_P, _Fin, _Fout))
    def _(t):
        return list(_T().feature_relu_forward(t["x"], t["w"], t["b"], with_hb=True))

    @case(f"feature_relu_backward[{_P}x{_Fin}x{_Fout}]", ["feature_relu_backward"], _feature_inputs(_P, _Fin, _Fout))
    def _(t):
        h = _T().feature_relu_forward(t["x"], t["w"], t["b"])[0]
        return list(_T().feature_relu_backward(t["g"], h, t["x"], t["w"]))


GEMM_SHAPE = (700, 640, 128)  # test_gemm_f32's (P, N, K) = (700, 640, 128)


def _rocblas_inputs(seed):
    g = _g(seed)
    P, N, K = GEMM_SHAPE
    return _od(w=torch.randn(N, K, generator=g) / N ** 0.5, dy=torch.randn(P, N, generator=g),
               x=torch.randn(P, K, generator=g))


# exact unless two default-stream runs differ on the parent commit: the handles disallow atomics, so rocBLAS's own
# pick is a deterministic kernel (test_train_step_deterministic rests on the same)
@case("gemm_f32", ["gemm_f32"], _rocblas_inputs)
def _(t):
    T = _T()
    P, N, K = GEMM_SHAPE
    dev = t["w"].device
    out = torch.empty(P, K, device=dev)           # out^T (K x P) = w^T (K x N) . dy^T (N x P)
    T.gemm_f32(t["w"], t["dy"], out, False, False, K, P, N, K, N, K, 1, 0, 0, 0, False)
    S, c = 2, 350                                 # strided batches: part_s^T (K x N) = x_s^T (K x c) . dy_s (c x N)
    parts = torch.empty(S, N, K, device=dev)
    T.gemm_f32(t["x"], t["dy"], parts, False, True, K, N, c, K, N, K, S, c * K, c * N, N * K, False)
    hb, db = t["x"].to(torch.bfloat16), t["dy"].to(torch.bfloat16)
    pb = torch.empty(N, K, device=dev)
    T.gemm_f32(hb, db, pb, False, True, K, N, P, K, N, K, 1, 0, 0, 0, False)
    return [out, parts, pb]


# ---- HexPlane, inference, voxels --------------------------------------------------------------------------------------
HEX_F, HEX_N = 16, 2000
HEX_RESOS = [(64, 64, 64, 25), (128, 128, 128, 25)]


def hex_sizes():
    import hexplane_path_scenes as HP
    return HP.sizes_of(HEX_RESOS)  # (W, H) of the 12 planes


def _hex_inputs(seed):
    """half the points spread over the field (a workgroup's cells overflow the LDS window: the direct path), half
    in one small box at one time (the window path); test_streams_gpu.py counts both from the route rule"""
    g = _g(seed)
    n = HEX_N // 2
    spread = torch.rand(n, 4, generator=g) * 2.2 - 1.1   # incl. border-clipped coordinates
    centre = torch.rand(1, 4, generator=g) - 0.5
    box = centre + 0.02 * (torch.rand(HEX_N - n, 4, generator=g) - 0.5)
    box[:, 3] = centre[0, 3]
    out = _od(pts=torch.cat([spread, box])[torch.randperm(HEX_N, generator=g)].contiguous(),
              dfeat=torch.randn(HEX_N, 2 * HEX_F, generator=g), xyz=torch.randn(HEX_N, 3, generator=g),
              time=torch.rand(HEX_N, 1, generator=g), aabb=torch.tensor([[1.5, 1.4, 1.6], [-1.5, -1.3, -1.6]]) +
              0.1 * torch.rand(2, 3, generator=g), dpts=torch.randn(HEX_N, 4, generator=g),
              add=torch.randn(HEX_N, 3, generator=g), dloss=torch.rand(1, generator=g) + 0.5)
    for i, (W, H) in enumerate(hex_sizes()):
        out[f"plane_{i:02d}"] = torch.rand(1, HEX_F, H, W, generator=g) * 1.1 + 0.1
        out[f"grad_{i:02d}"] = torch.randn(1, HEX_F, H, W, generator=g)
    return out


@case("hexplane_forward", ["hexplane_forward"], _hex_inputs)
def _(t):
    feat, packed, order = _T().hexplane_forward(t["pts"], _lst(t, "plane_"))
    feat2, _, order2 = _T().hexplane_forward(t["pts"], _lst(t, "plane_"), order)  # a kept order
    return [feat, packed, order, feat2]


@case("hexplane_forward_packed", ["hexplane_forward_packed"], _hex_inputs)
def _(t):
    feat, packed, order = _T().hexplane_forward(t["pts"], _lst(t, "plane_"))
    sizes = hex_sizes()
    return [_T().hexplane_forward_packed(t["pts"], packed, HEX_F, [w for w, h in sizes], [h for w, h in sizes], order)]


@case("hexplane_backward", ["hexplane_backward", "hexplane_backward_plan"], _hex_inputs)
def _(t):
    planes = _lst(t, "plane_")
    feat, packed, order = _T().hexplane_forward(t["pts"], planes)
    dpts, grads = _T().hexplane_backward(t["pts"], planes, packed, t["dfeat"], order)
    plan = torch.tensor(_T().hexplane_backward_plan(HEX_F), dtype=torch.int64, device=dpts.device)  # a host query
    return [dpts, *grads, plan]


@case("hexplane_points", ["hexplane_points"], _hex_inputs)
def _(t):
    one = t["time"][:1].expand(HEX_N, 1)  # one timestamp broadcast (stride 0), as a training view gives it
    return [_T().hexplane_points(t["xyz"], t["time"], t["aabb"]), _T().hexplane_points(t["xyz"], one, t["aabb"])]


@case("hexplane_points_backward", ["hexplane_points_backward"], _hex_inputs)
def _(t):
    return [_T().hexplane_points_backward(t["dpts"], t["aabb"])]


@case("hexplane_points_backward[add]", ["hexplane_points_backward"], _hex_inputs)
def _(t):
    return [_T().hexplane_points_backward(t["dpts"], t["aabb"], t["add"])]


def _reg_weights(n):
    ws = [0.01 if i % 6 in (2, 4, 5) else 0.0002 for i in range(n)]   # time planes: smoothness; space planes: TV
    wl = [0.0001 if i % 6 in (2, 4, 5) else 0.0 for i in range(n)]
    return ws, wl


@case("hexplane_reg_forward", ["hexplane_reg_forward"], _hex_inputs)
def _(t):
    planes = _lst(t, "plane_")
    return [_T().hexplane_reg_forward(planes, *_reg_weights(len(planes)))]


@case("hexplane_reg_backward", ["hexplane_reg_backward"], _hex_inputs)
def _(t):
    planes = _lst(t, "plane_")
    return list(_T().hexplane_reg_backward(planes, *_reg_weights(len(planes)), t["dloss"]))


@case("hexplane_reg_accumulate", ["hexplane_reg_accumulate"], _hex_inputs)
def _(t):
    planes, grads = _lst(t, "plane_"), _lst(t, "grad_")
    ws, wl = _reg_weights(len(planes))
    _T().hexplane_reg_accumulate(planes, grads, ws, wl, t["dloss"])
    v = _T().hexplane_reg_accumulate(planes, grads, ws, wl, t["dloss"], with_value=True, base=t["dloss"])
    return [v, *grads]


INFER_P, INFER_F, INFER_W, INFER_K = 777, 32, 64, 16
INFER_ROLES, INFER_N = (0, 1, 2, 3, 4), (3, 3, 4, 1, 48)


def _infer_inputs(seed):
    g = _g(seed)
    P, F, W, K, k = INFER_P, INFER_F, INFER_W, INFER_K, len(INFER_N)
    rn = lambda *s: torch.randn(*s, generator=g)
    out = _od(feat=rn(P, F), wf=rn(W, F) / F ** 0.5, bf=rn(W) * 0.1, w1=rn(k * W, W) / W ** 0.5, b1=rn(k * W) * 0.1,
              xyz=rn(P, 3), s=rn(P, 3), r=rn(P, 4), o=rn(P, 1), f_dc=rn(P, 1, 3), f_rest=rn(P, K - 1, 3))
    for i, n in enumerate(INFER_N):
        out[f"w2_{i}"] = rn(n, W) / W ** 0.5
        out[f"b2_{i}"] = rn(n) * 0.1
    return out


@case("deform_infer", ["deform_infer"], _infer_inputs)
def _(t):
    args = (t["feat"], t["wf"], t["bf"], t["w1"], t["b1"], _lst(t, "w2_"), _lst(t, "b2_"), list(INFER_ROLES), t["xyz"],
            t["s"], t["r"], t["o"], t["f_dc"], t["f_rest"])
    return list(_T().deform_infer(*args, True)) + list(_T().deform_infer(*args, False))


def _voxel_inputs(seed):
    import voxel_refs as VR
    pts, cols = VR.clustered_cloud(5000, seed=seed)
    return _od(points=torch.tensor(pts), colors=torch.tensor(cols))


@case("voxel_downsample", ["voxel_downsample"], _voxel_inputs)
def _(t):
    p, c, n = _T().voxel_downsample(t["points"], t["colors"], 0.05)
    p2, c2, n2 = _T().voxel_downsample(t["points"], None, 0.05)
    assert c2 is None
    return [p, c, n, p2, n2]


# ---- scratch growth: the ticket scratch made, reused and regrown under a non-default key -----------------------------
def _growth_inputs(seed):
    g = _g(seed)
    out = _od(xs=torch.rand(4 * 2048, generator=g), ys=torch.rand(4 * 2048, generator=g),
              xl=torch.rand(3, 600, 800, generator=g), yl=torch.rand(3, 600, 800, generator=g))
    for i in range(6):
        out[f"small_{i}"] = torch.rand(1, 4, 9, 9, generator=g)
        out[f"large_{i}"] = torch.rand(1, 16, 150, 128, generator=g)
    return out


@case("scratch_growth", ["l1_loss_grad", "hexplane_reg_forward"], _growth_inputs)
def _(t):
    T = _T()
    ws, wl = _reg_weights(6)
    out = []
    for x, y, planes in ((t["xs"], t["ys"], _lst(t, "small_")), (t["xs"], t["ys"], _lst(t, "small_")),
                         (t["xl"], t["yl"], _lst(t, "large_"))):   # made, reused, regrown
        out += list(T.l1_loss_grad(x, y, 1.0))
        out.append(T.hexplane_reg_forward(planes, ws, wl))
    return out


# ---- what has no case -------------------------------------------------------------------------------------------------
EXCLUDED = {
    "version": "returns a string; launches nothing",
    "set_profiling": "sets a host flag; launches nothing (its stage marks time the caller's stream and are not results)",
    "last_timings": "reads the host-side stage times; its values are timings",
    "debug_backward_occupancy": "a host occupancy query; launches nothing",
    "gemm_tuned": "lists the tuner's choices, which come from timing; launches nothing",
}

CASE_TABLE = collections.OrderedDict()
for _c in CASES.values():
    for _e in _c.entries:
        CASE_TABLE.setdefault(_e, []).append(_c.name)

SECOND_STREAM = ("l1_loss_grad", "ssim_forward", "gemm_f32", "rasterize_gaussians[sh]")
SECOND_DEVICE = ("rasterize_gaussians[sh]", "rasterize_gaussians_backward", "distCUDA2", "l1_loss_grad",
                 "hexplane_forward", "hexplane_backward", "heads_block_forward[777x64]", "adam_step", "voxel_downsample")


# ---- the two controls: valid-memory races that produce wrong values and nothing else ---------------------------------
def _control_inputs(seed):
    return _od(x=torch.randn(4096, generator=_g(seed)))


def bad_early(t):
    """reads its input on the null stream from inside the caller's stream context: before the caller's stream has
    produced it"""
    with torch.cuda.stream(torch.cuda.default_stream(t["x"].device)):
        return [t["x"] * 2]


def bad_late(t):
    """allocates its output on the caller's stream and fills it on the null stream: after the caller has read it"""
    out = torch.zeros_like(t["x"])
    with torch.cuda.stream(torch.cuda.default_stream(t["x"].device)):
        torch.mul(t["x"], 2, out=out)
    return [out]


def good(t):
    return [t["x"] * 2]


CONTROL_EARLY = Case("control: early reader", (), _control_inputs, bad_early)
CONTROL_LATE = Case("control: late writer", (), _control_inputs, bad_late)
CONTROL_GOOD = Case("control: correct", (), _control_inputs, good)
