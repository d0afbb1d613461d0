"""The HIP rasterizer and distCUDA2 against RECORDED RUNS OF THE REFERENCE'S OWN CODE (tests/golden/ref_raster_*.npz,
ref_knn_vectors.npz; tests/golden/make_raster_reference_vectors.py made them from the reference's CUDA sources built for
the host, tests/test_reference_run.py holds the oracle to the same files on the CPU).

Everything here reads tests/golden/ only.  The bars are oracle/parity.py's, unchanged, with the fixture arrays in the
oracle's place.  No flip allowance is needed or given: `oracle.flip_bounds` on each scene, computed here, must flag
nothing and bound every change by zero (the fixture scenes were chosen so; asserted before the comparison).
  num_rendered, radii                exact
  colour, depth, 8 gradients         parity.check
  final_T                            within IMG_SHARP of the reference's accum_alpha
  n_contrib                          exact, against the quantity the HIP forward stores under that name.  The reference
                                     stores the 1-based list position of the last splat that BLENDED into the pixel; the
                                     HIP forward (csrc/render.hip) stores the backward's bound instead: the position of the
                                     TERMINATING splat, or the list's length for a pixel that never terminated, and both
                                     in ITS OWN tile list, from which exact culling has dropped the splats that reach no
                                     pixel of the tile.  The two differ by design (only skipped splats lie between them,
                                     so the reverse walk is the same), and a direct comparison fails on every scene:
                                     depth_ties_small's first pixel holds 38 where the reference holds 19.  So the
                                     reference's decisions are replayed from the fixture's recorded state
                                     (reference_scenes.replay_walk; the replay must give the recorded n_contrib on every
                                     pixel, here and in tests/test_reference_run.py) and carried over to the HIP lists
                                     (debug_tile_lists): every HIP list must be a subsequence of the reference's list
                                     that keeps every splat the reference blends in the tile, and the HIP value must be,
                                     on every pixel, the position in that list of the splat at which the reference's walk
                                     terminates, or the list's length.
  the autograd API                   GaussianRasterizer on one SH scene and on the colors_precomp + cov3D_precomp scene
                                     (the route gaussian_renderer takes): every leaf's .grad under the same bars
  simple_knn._C.distCUDA2            bit for bit: the CPU test finds the oracle bitwise equal to the reference run, and
                                     the HIP path is bitwise equal to the oracle (tests/test_knn.py)
"""
import os

import numpy as np
import pytest
import torch

import reference_scenes as S
from gpu_helpers import c_backward, c_forward, o_bounds, o_forward, to_dev
from oracle import parity as PAR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FX = {}


@pytest.fixture(scope="module")
def C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def recorded(O, name):
    """the fixture, its scene, and the (zero) flip bounds of the scene from the oracle, made once"""
    if name not in _FX:
        with np.load(os.path.join(GOLDEN, f"ref_raster_{name}.npz")) as f:
            fx = {k: f[k] for k in f.files}
        sc = S.scene_of(fx, name)
        s = sc["s"]
        nr, _, _, radii, st = o_forward(O, s, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
        bounds = o_bounds(O, s, st, radii, fx["g"], colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
        assert not bounds["pflag"].any() and not bounds["gflag"].any(), f"{name}: a near-threshold decision"
        assert not bounds["pix_rad"].any() and not bounds["depth_rad"].any()
        assert not any(np.asarray(r).any() for r in bounds["grad_rad"]), f"{name}: a flip bound is not zero"
        _FX[name] = dict(fx=fx, sc=sc, bounds=bounds)
    return _FX[name]


def _tensors(sc, dev):
    d = to_dev(sc["s"], dev)
    col = None if sc["colors"] is None else torch.tensor(sc["colors"], device=dev)
    cov = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
    return d, col, cov


@pytest.mark.parametrize("name", S.FIXTURES)
def test_hip_matches_the_recorded_reference_run(C, oracle, dev, name):
    r = recorded(oracle, name)
    fx, sc = r["fx"], r["sc"]
    s = sc["s"]
    d, col, cov = _tensors(sc, dev)
    fwd = c_forward(C, s, d, colors=col, cov3D=cov, use_sh=sc["use_sh"])
    grads = c_backward(C, s, d, fwd, torch.tensor(fx["g"], device=dev), colors=col, cov3D=cov, use_sh=sc["use_sh"])
    torch.cuda.synchronize()
    assert fwd[0] == int(fx["num_rendered"]), f"num_rendered {fwd[0]} != the reference's {int(fx['num_rendered'])}"
    assert np.array_equal(fwd[3].cpu().numpy(), fx["radii"]), "radii differ"
    PAR.check(fwd[1].cpu().numpy(), fwd[2].cpu().numpy(), [a.cpu().numpy() for a in grads], fx["color"], fx["depth"],
              [fx[k] for k in PAR.GRAD_NAMES], r["bounds"], pix_frac=0.0, gauss_frac=0.0)
    if name == "sh0_m25":
        assert tuple(grads[5].shape) == (len(fx["radii"]), 25, 3) and not bool(grads[5][:, 1:].any())


@pytest.mark.parametrize("name", S.FIXTURES)
def test_image_state_matches_the_recorded_reference_run(C, oracle, dev, name):
    from test_gpu_parity import _final_T
    from test_importance_gpu import _n_contrib
    r = recorded(oracle, name)
    fx, sc = r["fx"], r["sc"]
    s = sc["s"]
    d, col, cov = _tensors(sc, dev)
    fwd = c_forward(C, s, d, colors=col, cov3D=cov, use_sh=sc["use_sh"])
    torch.cuda.synchronize()
    n_contrib, _ = _n_contrib(dict(sc=sc, fwd=fwd))
    n_contrib = n_contrib.cpu().numpy().reshape(s["H"], s["W"])
    W, H = s["W"], s["H"]
    last, _, _, term_gid, blended = S.replay_walk(fx, W, H)
    assert np.array_equal(last, fx["st_n_contrib"])  # the replay is the reference's walk
    if fwd[0] == 0:
        assert not n_contrib.any()
    else:
        out = C.debug_tile_lists(fwd[4], fwd[5], fwd[6], len(fx["radii"]), W, H, fwd[0])
        ranges, gid = out[0].cpu().numpy().astype(np.int64), out[3].cpu().numpy().astype(np.int64)
        want = np.zeros((H, W), np.int64)
        gx = (W + 15) // 16
        for t, (a, b) in enumerate(ranges):
            mine = gid[a:b].tolist()
            theirs = fx["st_point_list"][int(fx["st_ranges"][t, 0]):int(fx["st_ranges"][t, 1])].tolist()
            at = [theirs.index(g) for g in mine]  # ValueError: a splat the reference's list does not hold
            assert at == sorted(set(at)), f"tile {t}: not a subsequence of the reference's list"
            assert blended[t] <= set(mine), f"tile {t}: a splat that blends in the reference run was culled"
            y0, x0 = 16 * (t // gx), 16 * (t % gx)
            tg = term_gid[y0:y0 + 16, x0:x0 + 16]
            want[y0:y0 + 16, x0:x0 + 16] = [[len(mine) if g < 0 else mine.index(g) for g in row] for row in tg]
        assert np.array_equal(n_contrib, want), "n_contrib is not the terminating splat's position in the tile's list"
    if name == "term2":
        assert (term_gid >= 0).sum() > 100
    err =float(np.abs(_final_T(fwd[6], s["W"], s["H"]).astype(np.float64) - fx["st_final_T"]).max())
    print(f"\n[reference run] {name}: final_T within {err:.2e} of the reference's accum_alpha")
    assert err <= PAR.IMG_SHARP


@pytest.mark.parametrize("name", ["sh3_m16", "indef_small_colors"])
def test_autograd_api_matches_the_recorded_reference_run(oracle, dev, name):
    import diff_gaussian_rasterization as dgr
    r = recorded(oracle, name)
    fx, sc = r["fx"], r["sc"]
    s = sc["s"]
    d, col, cov = _tensors(sc, dev)
    settings = dgr.GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=d["bg"],
        scale_modifier=s["scale_modifier"], viewmatrix=d["viewmatrix"], projmatrix=d["projmatrix"],
        sh_degree=s["sh_degree"], campos=d["campos"], prefiltered=False, debug=False)
    leaf = lambda t: t.clone().requires_grad_(True)
    means3D, opac = leaf(d["means3D"]), leaf(d["opacities"])
    means2D = torch.zeros_like(means3D, requires_grad=True)
    leaves = {"dL_dmeans3D": means3D, "dL_dmeans2D": means2D, "dL_dopacity": opac}
    kw = {}
    if sc["use_sh"]:
        kw["shs"] = leaves["dL_dsh"] = leaf(d["shs"])
    else:
        kw["colors_precomp"] = leaves["dL_dcolors"] = leaf(col)
    if cov is None:
        kw["scales"] = leaves["dL_dscales"] = leaf(d["scales"])
        kw["rotations"] = leaves["dL_drotations"] = leaf(d["rotations"])
    else:
        kw["cov3D_precomp"] = leaves["dL_dcov3D"] = leaf(cov)
    color, radii, depth = dgr.GaussianRasterizer(settings)(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    color.backward(torch.tensor(fx["g"], device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), fx["radii"])
    names = [k for k in PAR.GRAD_NAMES if k in leaves]
    assert len(names) == (6 if name == "sh3_m16" else 5)
    rads = [r["bounds"]["grad_rad"][PAR.GRAD_NAMES.index(k)] for k in names]
    PAR.check(color.detach().cpu().numpy(), depth.detach().cpu().numpy(), [leaves[k].grad.cpu().numpy() for k in names],
              fx["color"], fx["depth"], [fx[k] for k in names], r["bounds"], o_rads=rads, pix_frac=0.0, gauss_frac=0.0,
              names=names)


def test_distcuda2_matches_the_recorded_reference_run():
    from simple_knn._C import distCUDA2
    with np.load(os.path.join(GOLDEN, "ref_knn_vectors.npz")) as f:
        names = sorted(k[:-2] for k in f.files if k.endswith("_x"))
        assert len(names) == 10
        for n in names:
            got = distCUDA2(torch.from_numpy(f[f"{n}_x"]).cuda())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got.cpu().numpy(), f[f"{n}_d"], err_msg=n)
