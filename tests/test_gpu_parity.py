"""GPU parity: the HIP path (through the `_C` binding over the C ABI) against the CPU oracle.

The bars (north_star's 1e-4 on RGB/depth and 1e-3 on gradients, per element, plus sharper bars at the
measured maxima, and the flip-flag allowances for the blend's two discrete thresholds) are defined and
asserted in oracle/parity.py; every case prints its report, so each config's measured maxima are in
the log.
"""
import math

import numpy as np
import pytest
import torch

from gpu_helpers import c_backward, c_forward, o_backward, o_bounds, o_forward, to_dev
from gs4d_train.synthetic import make_scene, make_upstream_grad
from oracle import parity as PAR

pytestmark = pytest.mark.gpu
# measured flagged shares above oracle/parity.py's defaults (round 5 bands): the train-like scene's large
# splats (1.5 % of the Gaussians have a near-threshold pixel); the 2^20-tile grid's few hundred splats with
# huge footprints (17 %); the long-tile scene's thousands of faint splats per pixel (0.7 % of the pixels)
TRAIN_LIKE_GAUSS_FRAC = 0.03
GRID_GAUSS_FRAC = 0.35
LONG_TILES_PIX_FRAC = 0.015


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import diff_gaussian_rasterization as dgr
    return dgr._C


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _check(C, O, s, dev, colors=None, cov3D=None, use_sh=True, degree=None, report=None,
           pix_frac=PAR.FLIP_PIX_FRAC, gauss_frac=PAR.FLIP_GAUSS_FRAC):
    d = to_dev(s, dev)
    col_t = None if colors is None else torch.tensor(colors, device=dev)
    cov_t = None if cov3D is None else torch.tensor(cov3D, device=dev)
    fwd = c_forward(C, s, d, colors=col_t, cov3D=cov_t, use_sh=use_sh, degree=degree)
    torch.cuda.synchronize()
    nr, color, depth, radii, st = o_forward(O, s, colors=colors, cov3D=cov3D, use_sh=use_sh, degree=degree)
    assert fwd[0] == nr, f"num_rendered {fwd[0]} != oracle {nr}"
    assert np.array_equal(fwd[3].cpu().numpy(), radii), "radii differ"
    g, _ = make_upstream_grad(color)
    g = g * (3 * s["W"] * s["H"])
    grads_c = c_backward(C, s, d, fwd, torch.tensor(g, device=dev), colors=col_t, cov3D=cov_t, use_sh=use_sh,
                         degree=degree)
    torch.cuda.synchronize()
    grads_o = o_backward(O, s, st, radii, g, colors=colors, cov3D=cov3D, use_sh=use_sh, degree=degree)
    bounds = o_bounds(O, s, st, radii, g, colors=colors, cov3D=cov3D, use_sh=use_sh, degree=degree)
    res = PAR.check(fwd[1].cpu().numpy(), fwd[2].cpu().numpy(), [a.cpu().numpy() for a in grads_c], color, depth,
                    grads_o, bounds, pix_frac=pix_frac, gauss_frac=gauss_frac)
    res["L"] = nr
    if report is not None:
        report.append(res)
    return fwd, grads_c


@pytest.mark.parametrize("P,W,H,seed,deg", [
    (3000, 160, 96, 0, 3),
    (20000, 400, 400, 1, 3),     # BASELINE config C1 size
    (5000, 257, 129, 2, 2),      # W, H not multiples of 16
    (4000, 200, 120, 3, 1),
    (4000, 200, 120, 4, 0),
    (1, 33, 21, 5, 3),
])
def test_parity_sh(C, oracle, dev, P, W, H, seed, deg):
    s = make_scene(P, W, H, seed=seed, sh_degree=deg)
    _check(C, oracle, s, dev)


@pytest.mark.parametrize("M,deg", [(4, 1), (9, 2), (25, 3)])
def test_parity_sh_row_widths(C, oracle, dev, M, deg):
    """Coefficient rows other than the 16 of degree 3 (the SH backward's scalar staging path): rows of
    exactly (D+1)^2, and 25 > 16 coefficients whose tail gets zero gradients (backward.cu:20-139 writes
    only the (D+1)^2 it uses; the dL_dsh tensor starts zeroed, rasterize_points.cu)."""
    s = make_scene(2000, 160, 96, seed=30 + M, sh_degree=deg)
    sh = np.zeros((2000, M, 3), np.float32)
    k = min(M, 16)
    sh[:, :k] = s["shs"][:, :k]
    if M > 16:
        sh[:, 16:] = np.random.default_rng(M).normal(0, 0.1, (2000, M - 16, 3))
    s["shs"] = sh
    _, grads = _check(C, oracle, s, dev)
    dsh = grads[5]  # (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, ...)
    assert tuple(dsh.shape) == (2000, M, 3)
    assert not bool(dsh[:, (deg + 1) ** 2:].any())


def test_parity_bg_black(C, oracle, dev):
    s = make_scene(3000, 160, 96, seed=7)
    s["bg"] = np.zeros(3, np.float32)
    _check(C, oracle, s, dev)


def test_parity_colors_precomp(C, oracle, dev):
    s = make_scene(3000, 160, 96, seed=8)
    colors = np.random.default_rng(9).uniform(0, 1, (3000, 3)).astype(np.float32)
    _check(C, oracle, s, dev, colors=colors, use_sh=False)


def test_parity_cov3D_precomp(C, oracle, dev):
    s = make_scene(3000, 160, 96, seed=10)
    q = s["rotations"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Cm = np.einsum("pij,pj,pkj->pik", R, s["scales"].astype(np.float64) ** 2, R)
    cov3D = np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], 1).astype(
        np.float32)
    _check(C, oracle, s, dev, cov3D=cov3D)


def test_parity_scale_modifier_and_big_splats(C, oracle, dev):
    s = make_scene(800, 160, 96, seed=12, log_scale=math.log(0.2))
    s["scale_modifier"] = 0.7
    _check(C, oracle, s, dev)


def test_parity_frustum_clamp_and_independent_fovy(C, oracle, dev):
    """Splats centred beyond the 1.3 tan_fov frustum clamp of computeCov2D (forward.cu:83-87, backward.cu:165-170,
    262-264) that still overlap the image, seen by a rotated camera whose fovy is independent of fovx and the aspect
    ratio (focal_x != focal_y): the small scenes of tests/rule_scenes.py at scale, against the oracle."""
    import rule_scenes as RS
    s = RS.view_with_camera(make_scene(3000, 160, 96, seed=32, spread=1.7, log_scale=math.log(0.1)), rescale_y=False)
    fx, fy = s["W"] / (2 * s["tanfovx"]), s["H"] / (2 * s["tanfovy"])
    assert abs(fx - fy) > 0.05 * fx
    fwd, _ = _check(C, oracle, s, dev)
    view = s["viewmatrix"].astype(np.float64).reshape(4, 4)
    t = (np.c_[s["means3D"].astype(np.float64), np.ones(3000)] @ view)[:, :3]
    clamped = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * s["tanfovx"]) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * s["tanfovy"])
    assert int((clamped & (fwd[3].cpu().numpy() > 0)).sum()) >= 100


def test_parity_opaque_stack_termination(C, oracle, dev):
    """Many nearly opaque splats: exercises the 0.99 clamp and the T < 1e-4 early exit."""
    s = make_scene(6000, 128, 128, seed=13, log_scale=math.log(0.1))
    s["opacities"] = np.full_like(s["opacities"], 0.995)
    _check(C, oracle, s, dev)


def test_parity_long_tiles(C, oracle, dev):
    """Tiles holding more instances than one workgroup sorts in LDS (2048): 30k large, faint splats
    over a 12-tile image (9k-16k instances per tile) exercise the per-tile sort's global merge steps."""
    s = make_scene(30000, 64, 48, seed=19, log_scale=math.log(0.3))
    s["opacities"] = np.full_like(s["opacities"], 0.03)
    # thousands of faint splats per pixel: 0.7 % of the pixels hold a near-threshold decision
    fwd, _ = _check(C, oracle, s, dev, pix_frac=LONG_TILES_PIX_FRAC)
    assert fwd[0] > 12 * 4096


def test_parity_depth_ties(C, oracle, dev):
    """Groups of Gaussians at exactly the same depth: within a tile the reference orders ties by id."""
    s = make_scene(4000, 160, 96, seed=20)
    s["means3D"][:, 2] = np.round(s["means3D"][:, 2] * 4) / 4  # a handful of distinct depths
    _check(C, oracle, s, dev)


def test_empty_and_all_culled(C, oracle, dev):
    s = make_scene(100, 64, 48, seed=14)
    d = to_dev(s, dev)
    s0 = dict(s)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        s0[k] = s[k][:0]
    d0 = to_dev(s0, dev)
    nr, color, depth, radii, gb, bb, ib = c_forward(C, s0, d0)
    assert nr == 0 and radii.numel() == 0 and not color.any() and not depth.any()
    # everything behind the near plane: background everywhere, zero gradients
    s["means3D"][:, 2] = 0.1
    _check(C, oracle, s, dev)
    fwd = c_forward(C, s, to_dev(s, dev))
    assert fwd[0] == 0
    assert torch.allclose(fwd[1], torch.ones_like(fwd[1]))


def test_prefiltered_raises(C, dev):
    s = make_scene(100, 64, 48, seed=15)
    s["means3D"][0, 2] = 0.1
    with pytest.raises(RuntimeError, match="prefiltered"):
        c_forward(C, s, to_dev(s, dev), prefiltered=True)


def test_mark_visible(C, oracle, dev):
    s = make_scene(1000, 64, 48, seed=16)
    s["means3D"][::3, 2] = np.linspace(-1, 0.2, len(s["means3D"][::3, 2]))
    d = to_dev(s, dev)
    vis = C.mark_visible(d["means3D"], d["viewmatrix"], d["projmatrix"]).cpu().numpy()
    assert np.array_equal(vis, oracle.mark_visible(s["means3D"], s["viewmatrix"], s["projmatrix"]))


def test_deterministic_bitwise(C, dev):
    """No float atomics anywhere: two runs give identical bits (the reference cannot)."""
    s = make_scene(20000, 400, 400, seed=17)
    d = to_dev(s, dev)
    outs = []
    for _ in range(2):
        fwd = c_forward(C, s, d)
        g = torch.sign(fwd[1] - 0.5)
        grads = c_backward(C, s, d, fwd, g)
        outs.append([fwd[1], fwd[2]] + list(grads))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_metric_config_properties(C, oracle, dev):
    """BASELINE metric size (100k Gaussians, 1352x1014): num_rendered / radii exact, images and
    gradients at parity with the oracle."""
    s = make_scene(100_000, 1352, 1014, seed=0)
    _check(C, oracle, s, dev)


@pytest.mark.parametrize("cfg", ["c2_800", "c4_per_view", "c5_broom"])
def test_large_configs(C, oracle, dev, cfg):
    """BASELINE configs C2 (100k Gaussians, 800x800), C4 (300k Gaussians, 1352x1014, one view of the
    8-GPU run) and C5 (1M Gaussians, 960x536): full parity with the oracle at those sizes."""
    from gs4d_train.synthetic import CONFIGS
    P, W, H = CONFIGS[cfg]
    s = make_scene(P, W, H, seed=21)
    _check(C, oracle, s, dev)


def test_train_like_scene(C, oracle, dev):
    """The bench's second workload (make_train_like_scene: a k-NN-initialised point cloud as
    create_from_pcd leaves it, ~1,200 instances per touched tile, runs sorted by tile_sort_kernel)."""
    from gs4d_train.synthetic import make_train_like_scene
    s = make_train_like_scene(100_000, 1352, 1014, seed=0)
    _check(C, oracle, s, dev, gauss_frac=TRAIN_LIKE_GAUSS_FRAC)


def test_parity_mid_tiles(C, oracle, dev):
    """Tile runs between 256 and 2048+ instances, the regime of a training scene's early iterations
    (dense, large, faint splats): sorted in LDS by tile_sort_kernel before the forward blends them."""
    s = make_scene(20000, 192, 128, seed=22, log_scale=math.log(0.08))
    s["opacities"] = np.full_like(s["opacities"], 0.1)
    fwd, _ = _check(C, oracle, s, dev)
    assert fwd[0] > 96 * 256


def test_capacity_prediction_both_ways(C, oracle, dev):
    """Scenes of very different sizes back to back through the same caller-owned buffers: the binning
    buffer is resized from the host's exact num_rendered on every call (the Resizer of torch_glue.cpp, as
    rasterizer_impl.cu:283-290 does), so a scene with ~20x more instances than its predecessor grows it
    and the small scene after it runs in a buffer carved for its own size; all three must match the
    oracle, backward included (the backward re-carves the buffers from num_rendered)."""
    small = make_scene(2000, 256, 192, seed=23)
    big = make_scene(40000, 512, 384, seed=24, log_scale=math.log(0.05))
    _check(C, oracle, small, dev)
    fwd_big, _ = _check(C, oracle, big, dev)
    fwd_small, _ = _check(C, oracle, small, dev)
    assert fwd_big[0] > 20 * fwd_small[0]


def test_autograd_api(dev, oracle):
    """Through GaussianRasterizer + autograd, exactly as gaussian_renderer/__init__.py calls it."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import diff_gaussian_rasterization as dgr
    s = make_scene(3000, 160, 96, seed=18)
    d = to_dev(s, dev)
    settings = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=1.0, viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"], sh_degree=3, campos=d["campos"],
        prefiltered=False, debug=False)
    raster = dgr.GaussianRasterizer(settings)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    screenspace = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
    screenspace.retain_grad()
    img, radii, depth = raster(means3D=leaves["means3D"], means2D=screenspace, shs=leaves["shs"],
                               opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"])
    g, _ = make_upstream_grad(img.detach().cpu().numpy())
    (img * torch.tensor(g, device=dev)).sum().backward()
    nr, color, depth_o, radii_o, st = o_forward(oracle, s)
    go = o_backward(oracle, s, st, radii_o, g)
    bounds = o_bounds(oracle, s, st, radii_o, g)
    rad = bounds["grad_rad"]
    # the Python API's gradients: (means3D, shs, opacities, scales, rotations, means2D) against the
    # oracle's (dL_dmeans3D, dL_dsh, dL_dopacity, dL_dscales, dL_drotations, dL_dmeans2D)
    res = PAR.check(img.detach().cpu().numpy(), depth.detach().cpu().numpy(),
                    [leaves[k].grad.cpu().numpy() for k in ("means3D", "shs", "opacities", "scales", "rotations")]
                    + [screenspace.grad.cpu().numpy()], color, depth_o,
                    [go[3], go[5], go[2], go[6], go[7], go[0]], bounds,
                    o_rads=[rad[3], rad[5], rad[2], rad[6], rad[7], rad[0]],
                    names=["means3D", "shs", "opacities", "scales", "rotations", "means2D"])
    vis = raster.markVisible(leaves["means3D"].detach())
    assert vis.dtype == torch.bool and vis.shape == (3000,)


def _image_buffer_views(ib, W, H):
    """final_T, n_contrib, ranges and order carved from the forward's image buffer (capi.hip
    ImageState::carve: 256-byte aligned arrays in this order)."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    N = W * H
    al = lambda x: (x + 255) // 256 * 256
    base = al(ib.data_ptr()) - ib.data_ptr()
    raw = ib.cpu().numpy().view(np.uint8)
    off_r = base + 2 * al(4 * N)
    ranges = raw[off_r:off_r + 8 * T].view(np.uint32).reshape(T, 2)
    off_o = off_r + al(8 * T)
    order = raw[off_o:off_o + 4 * T].view(np.uint32)
    return ranges, order


@pytest.mark.parametrize("W,H", [(1352, 1014), (2304, 1296), (2048, 2048), (2400, 2000)])
def test_tile_order_longest_first(C, oracle, dev, W, H):
    """The blend kernels take tiles longest run first (tile_order_kernel): the order is a permutation
    of the tiles with non-increasing run lengths (capped at 1023).  2304x1296 has 11,664 tiles, more than
    the order kernel keeps in registers (8192), and is checked against the oracle as well; 2048x2048 has
    16,384, the counting binning's largest grid (64 KiB of LDS bins, binning.hip kCountMaxT); 2400x2000 has
    18,750, more than that: the radix-sort binning.
    The tile ranges partition the emitted instances in tile order, empty tiles (0, 0) as
    identifyTileRanges leaves them (rasterizer_impl.cu:116-138)."""
    s = make_scene(100_000 if W == 1352 else 3000, W, H, seed=25)
    if W == 1352:
        fwd = c_forward(C, s, to_dev(s, dev))
    else:
        fwd, _ = _check(C, oracle, s, dev)
    ranges, order = _image_buffer_views(fwd[6], W, H)
    T = ranges.shape[0]
    assert np.array_equal(np.sort(order), np.arange(T))
    lens = np.minimum(ranges[order, 1] - ranges[order, 0], 1023)
    assert np.all(np.diff(lens.astype(np.int64)) <= 0)
    ne = ranges[:, 1] > ranges[:, 0]
    assert np.all(ranges[~ne] == 0)
    r = ranges[ne].astype(np.int64)
    assert r[0, 0] == 0 and np.array_equal(r[1:, 0], r[:-1, 1])
    assert r[-1, 1] <= fwd[0]  # L' <= num_rendered


def test_view_matrix_layouts_agree(C, dev):
    """The reference's callers pass world_view_transform as a transposed (1, 4)-strided view, which the
    kernels read in place (gs4d_*_ex, view_transposed = 1); a contiguous copy of the same matrix takes
    the plain path.  Both must give bit-identical images, radii, gradients and visibility."""
    s = make_scene(5000, 200, 136, seed=26)
    d = to_dev(s, dev)
    vm_c = d["viewmatrix"].contiguous()
    vm_t = vm_c.t().contiguous().t()
    assert vm_t.stride() == (1, 4) and vm_c.stride() == (4, 1) and torch.equal(vm_t, vm_c)
    outs = []
    for vm in (vm_c, vm_t):
        dd = dict(d, viewmatrix=vm)
        fwd = c_forward(C, s, dd)
        grads = c_backward(C, s, dd, fwd, torch.sign(fwd[1] - 0.5))
        vis = C.mark_visible(dd["means3D"], vm, dd["projmatrix"])
        outs.append([fwd[1], fwd[2], fwd[3], vis] + list(grads))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_grid_of_2pow20_tiles(C, oracle, dev):
    """A grid of 2^20 tiles or more (16400 x 16400: 1,050,625 tiles): the emission locates a candidate in
    its rectangle by exact integer division there (Args.exact_div) instead of the float reciprocal, and
    the radix-sort binning takes 3 passes over the 21 tile bits.  num_rendered and radii exact, images
    and gradients against the oracle (a few hundred splats: the image is mostly background)."""
    s = make_scene(300, 16400, 16400, seed=27)
    d = to_dev(s, dev)
    fwd = c_forward(C, s, d)
    torch.cuda.synchronize()
    nr, color, depth, radii, st = o_forward(oracle, s)
    assert fwd[0] == nr and np.array_equal(fwd[3].cpu().numpy(), radii)
    g = np.sign(color - 0.5).astype(np.float32)
    grads_c = c_backward(C, s, d, fwd, torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    grads_o = o_backward(oracle, s, st, radii, g)
    bounds = o_bounds(oracle, s, st, radii, g)
    res = PAR.check(fwd[1].cpu().numpy(), fwd[2].cpu().numpy(), [a.cpu().numpy() for a in grads_c], color, depth,
                    grads_o, bounds, gauss_frac=GRID_GAUSS_FRAC)


def _final_T(ib, W, H):
    """final_T carved from the forward's image buffer (capi.hip ImageState::carve: first array)."""
    base = (ib.data_ptr() + 255) // 256 * 256 - ib.data_ptr()
    raw = ib.cpu().numpy().view(np.uint8)
    return raw[base:base + 4 * W * H].view(np.float32).reshape(H, W)


@pytest.mark.parametrize("cfg", ["metric", "c2_800", "train_like", "opaque"])
def test_flip_bands_cover_measured_operands(C, oracle, dev, cfg):
    """The near-threshold bands of oracle/parity.py are set from this measurement, not guessed:
      * alpha: for every (pixel, splat) pair of the oracle's walks with 255 alpha within 1e-4 mag of 1 (mag =
        1 + the magnitude of the power's terms at the pair, the oracle's near_alpha), the blend kernels' own o G
        (gs4d_debug_pair_alpha: the exact arithmetic of both blend kernels) differs from the oracle's by at
        most FLIP_BAND_ALPHA / 2 x mag, relative to 1/255;
      * termination: T(1 - alpha) is a product of the walk's (1 - alpha) factors, so its relative difference
        is bounded by the final transmittance's (every pixel whose decisions the oracle does not flag) plus
        the last factor's, measured on the pairs within 1e-2 of the termination threshold; that sum is at
        most FLIP_BAND_T / 2.
    Prints the measured maxima (DESIGN.md §5 quotes them)."""
    from gs4d_train.synthetic import CONFIGS, make_train_like_scene
    if cfg == "metric":
        s = make_scene(100_000, 1352, 1014, seed=0)
    elif cfg == "c2_800":
        P, W, H = CONFIGS[cfg]
        s = make_scene(P, W, H, seed=21)
    elif cfg == "train_like":
        s = make_train_like_scene(100_000, 1352, 1014, seed=0)
    else:  # many terminations
        s = make_scene(6000, 128, 128, seed=13, log_scale=math.log(0.1))
        s["opacities"] = np.full_like(s["opacities"], 0.995)
    d = to_dev(s, dev)
    fwd = c_forward(C, s, d)
    torch.cuda.synchronize()
    nr, color, depth, radii, st = o_forward(oracle, s)
    t = lambda a: torch.tensor(a, device=dev)

    def gpu_og(gid, px, py):
        return C.debug_pair_alpha(fwd[4], len(radii), s["W"], s["H"], t(gid), t(px), t(py))[0].cpu().numpy()
    gid, px, py, og, mag = oracle.near_pairs(st, 1e-4, kind=1)
    assert len(gid) > 0
    dev_a = np.abs(255.0 * gpu_og(gid, px, py).astype(np.float64) - 255.0 * og.astype(np.float64))
    d_alpha = float((dev_a / mag).max())  # per unit of the pair's magnitude factor (oracle near_alpha)
    T_gpu = _final_T(fwd[6], s["W"], s["H"])
    T_o = st.export()["final_T"]
    pflag, _ = oracle.flip_flags(st, PAR.FLIP_BAND_ALPHA, PAR.FLIP_BAND_T)
    ok = (pflag == 0) & (T_o > 0)
    d_T = float((np.abs(T_gpu.astype(np.float64) - T_o) / T_o)[ok].max())
    # T(1 - alpha) near 1e-4: the running product's relative difference (the final transmittance's bounds it)
    # plus the last factor's, |alpha_gpu - alpha_oracle| / (1 - alpha) measured on the near-termination pairs
    gid2, px2, py2, og2, _ = oracle.near_pairs(st, 1e-2, kind=2)
    d_om = 0.0
    if len(gid2):
        a_g = np.minimum(0.99, gpu_og(gid2, px2, py2).astype(np.float64))
        a_o = np.minimum(0.99, og2.astype(np.float64))
        d_om = float((np.abs(a_g - a_o) / (1.0 - a_o)).max())
    d_test_T = d_T + d_om
    print(f"{cfg}: {len(gid)} pairs within 1e-4 mag of 1/255: max |255 alpha_gpu - 255 alpha_oracle| = "
          f"{float(dev_a.max()):.3g}, per unit of mag {d_alpha:.3g} (band {PAR.FLIP_BAND_ALPHA:.3g}); final T max relative difference {d_T:.3g}, {len(gid2)} pairs within "
          f"1e-2 of termination: 1 - alpha {d_om:.3g}, test_T bound {d_test_T:.3g} (band {PAR.FLIP_BAND_T:.3g})",
          flush=True)
    assert d_alpha <= PAR.FLIP_BAND_ALPHA / 2
    assert d_test_T <= PAR.FLIP_BAND_T / 2


def _cov3d_of(s):
    q = s["rotations"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Cm = np.einsum("pij,pj,pkj->pik", R, s["scales"].astype(np.float64) ** 2, R)
    return np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], 1).astype(np.float32)


@pytest.mark.parametrize("mode", ["colors+scales_rotations", "shs+cov3D"])
def test_autograd_api_gradient_routing(C, dev, mode):
    """_RasterizeGaussians.backward returns eight gradients by position; test_autograd_api passes SH, scales and
    rotations only.  With colors_precomp + scales / rotations, and with shs + cov3D_precomp, each leaf's .grad is
    bitwise the tensor _C.rasterize_gaussians_backward returns for that quantity on the same inputs (the path the
    oracle tests hold), the leaves that are not passed get none, and a backward from the depth image alone leaves
    every .grad None (no gradient flows from depth, as in the reference)."""
    import diff_gaussian_rasterization as dgr
    s = make_scene(500, 96, 64)
    d = to_dev(s, dev)
    settings = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=float(s["scale_modifier"]), viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"],
        sh_degree=int(s["sh_degree"]), campos=d["campos"], prefiltered=False, debug=False)
    raster = dgr.GaussianRasterizer(settings)
    colors = torch.tensor(np.random.default_rng(9).uniform(0, 1, (500, 3)).astype(np.float32), device=dev)
    cov3D = torch.tensor(_cov3d_of(s), device=dev)
    use_colors = mode.startswith("colors")
    col_t, cov_t = (colors, None) if use_colors else (None, cov3D)

    def leaves():
        t = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
        t["colors_precomp"] = colors.clone().requires_grad_(True)
        t["cov3D_precomp"] = cov3D.clone().requires_grad_(True)
        return t
    passed = ["means3D", "means2D", "opacities"] + (["colors_precomp", "scales", "rotations"] if use_colors
                                                    else ["shs", "cov3D_precomp"])
    t = leaves()
    img, radii, depth = raster(**{k: t[k] for k in passed})
    g, _ = make_upstream_grad(img.detach().cpu().numpy())
    gt = torch.tensor(g, device=dev)
    (img * gt).sum().backward()
    fwd = c_forward(C, s, d, colors=col_t, cov3D=cov_t, use_sh=not use_colors)
    assert torch.equal(fwd[1], img.detach()) and torch.equal(fwd[2], depth.detach()) and torch.equal(fwd[3], radii)
    # (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    raw = dict(zip(("means2D", "colors_precomp", "opacities", "means3D", "cov3D_precomp", "shs", "scales", "rotations"),
                   c_backward(C, s, d, fwd, gt, colors=col_t, cov3D=cov_t, use_sh=not use_colors)))
    for k, leaf in t.items():
        if k in passed:
            assert leaf.grad is not None and leaf.grad.shape == leaf.shape, k
            assert torch.equal(leaf.grad, raw[k]), k
            assert k == "means2D" or bool(leaf.grad.any()), k
        else:
            assert leaf.grad is None, k
    t = leaves()
    img, radii, depth = raster(**{k: t[k] for k in passed})
    depth.sum().backward()
    assert all(leaf.grad is None for leaf in t.values())
