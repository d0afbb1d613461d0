"""CPU tests of the blend-weight importance boundary (no GPU calls): gs4d_importance is declared and exported and
refuses bad input with its status codes; gs4d_train.pruning.importance_mask on hand-made scores; and the properties
of tests/importance_refs.py that tests/test_importance_gpu.py relies on, through the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth_scenes as DS
import importance_refs as IR
import tile_list_scenes as TL
from gpu_helpers import o_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    return L


def test_header_declares_and_library_exports_gs4d_importance(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int gs4d_importance\s*\(([^;]*)\);", text, flags=re.S)
    assert m, "gs4d_importance is not declared (with its comment)"
    comment = re.sub(r"[\s*]+", " ", m.group(1))  # the comment's words, line breaks and their stars aside
    params = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    assert params == ["int P", "int width", "int height", "int num_rendered", "const char *geometry_buffer",
                      "const char *binning_buffer", "const char *image_buffer", "float *weight_sum",
                      "float *weight_max", "int32_t *pixel_count", "gs4d_alloc_fn scratch_alloc", "void *scratch_ctx",
                      "void *stream"]
    # the weight's reference lines, and that the reference returns no such quantity
    assert "forward.cu:357-358" in comment and "returns no such quantity" in comment
    assert "forward.cu:330-366" in comment and "bit for bit" in comment and "float atomics" in comment
    assert hasattr(lib, "gs4d_importance")


def _call(lib, P=4, W=16, H=16, R=8, geom=True, binning=True, image=True, wsum=True, wmax=True, count=True,
          alloc="null"):
    buf = (ctypes.c_float * 64)()
    some, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    p = lambda on: some if on else null
    calls = []

    def returns_null(ctx, n):
        calls.append(n)
        return None
    cb = ALLOC(returns_null) if alloc == "null" else ALLOC()
    i = ctypes.c_int
    st = lib.gs4d_importance(i(P), i(W), i(H), i(R), p(geom), p(binning), p(image), p(wsum), p(wmax), p(count), cb,
                             null, null)
    return st, lib.gs4d_last_error(), calls


def test_argument_errors_are_status_codes(lib):
    bad = [dict(P=-1), dict(W=0), dict(H=0), dict(W=-3), dict(R=-1), dict(geom=False), dict(binning=False),
           dict(image=False), dict(wsum=False), dict(wmax=False), dict(count=False), dict(alloc=None)]
    for kw in bad:
        st, msg, calls = _call(lib, **kw)
        assert st == 1 and msg.startswith(b"importance:"), (kw, st, msg)  # GS4D_ERR_ARG
        assert calls == [], kw                                            # refused before the scratch is asked for
    # the allocator returning NULL is GS4D_ERR_ALLOC; it was asked for the records of R slots and more
    st, msg, calls = _call(lib)
    assert st == 2 and msg.startswith(b"importance:") and len(calls) == 1 and calls[0] >= 8 * 16
    # P == 0 is GS4D_OK at once, whatever else is missing
    st, _, calls = _call(lib, P=0, W=0, H=0, geom=False, binning=False, image=False, wsum=False, wmax=False,
                         count=False, alloc=None)
    assert st == 0 and calls == []


def test_python_surface_exists_and_is_opt_in():
    import inspect

    import diff_gaussian_rasterization as dgr
    from gs4d_train import infer, pruning, train
    assert hasattr(dgr._C, "gaussian_importance") and callable(dgr.gaussian_importance)
    sig = inspect.signature(dgr.gaussian_importance)
    assert list(sig.parameters) == ["means3D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                                    "cov3D_precomp", "raster_settings", "antialiasing"]
    assert sig.parameters["antialiasing"].default is False
    assert list(inspect.signature(infer.importance).parameters) == ["state", "cameras", "antialiasing"]
    assert list(inspect.signature(pruning.prune_by_importance).parameters) == [
        "gaussians", "cameras", "min_max_weight", "keep_fraction", "by", "antialiasing"]
    assert "importance" not in inspect.getsource(train.train_step)  # the training loop calls it where it wants
    # P == 0 returns empty tensors without touching _C (CPU tensors would raise there)
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    out = dgr.gaussian_importance(torch.zeros(0, 3), torch.zeros(0, 1), shs=torch.zeros(0, 16, 3),
                                  scales=torch.zeros(0, 3), rotations=torch.zeros(0, 4), raster_settings=st)
    assert [tuple(t.shape) for t in out] == [(0,)] * 4
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32]
    with pytest.raises(RuntimeError):  # no CPU path
        dgr._C.gaussian_importance(torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8),
                                   torch.zeros(64, dtype=torch.uint8), 4, 4, 8, 8)


# ---- importance_mask ------------------------------------------------------------------------------------------------
def _scores():
    return {"sum": torch.tensor([5.0, 1.0, 3.0, 3.0, 0.0, 9.0], dtype=torch.float64),
            "max": torch.tensor([0.5, 0.004, 0.2, 0.3, 0.0, 0.009]),
            "count": torch.tensor([10, 2, 7, 7, 0, 1]), "views": torch.tensor([2, 1, 2, 2, 0, 1])}


def test_importance_mask_rules():
    from gs4d_train.pruning import importance_mask
    s = _scores()
    # RadSplat's rule alone: max < 0.01
    assert importance_mask(s, min_max_weight=0.01).tolist() == [False, True, False, False, True, True]
    assert importance_mask(s, min_max_weight=0.004).tolist() == [False, False, False, False, True, False]  # strict <
    # the ranking alone: top ceil(0.5 * 6) = 3 by sum are rows 5, 0 and, of the tied 2 and 3, the lower index
    assert importance_mask(s, keep_fraction=0.5).tolist() == [False, True, False, True, True, False]
    # ceil: 0.34 * 6 = 2.04 -> 3 rows kept; 1/3 -> 2 rows
    assert int((~importance_mask(s, keep_fraction=0.34)).sum()) == 3
    assert importance_mask(s, keep_fraction=2 / 6).tolist() == [False, True, True, True, True, False]
    # by another score; ties (rows 2 and 3 by count) again to the lower index
    assert importance_mask(s, keep_fraction=0.5, by="max").tolist() == [False, True, False, False, True, True]
    assert importance_mask(s, keep_fraction=2 / 6, by="count").tolist() == [False, True, False, True, True, True]
    # both rules are OR-ed: row 5 is in the top three by sum but its max is below the threshold
    assert importance_mask(s, min_max_weight=0.01, keep_fraction=0.5).tolist() == [False, True, False, True, True, True]
    # keep_fraction = 1 prunes nothing
    assert not importance_mask(s, keep_fraction=1.0).any()
    # all equal: the first rows win
    flat = {"sum": torch.zeros(5, dtype=torch.float64), "max": torch.zeros(5)}
    assert importance_mask(flat, keep_fraction=0.4).tolist() == [False, False, True, True, True]
    m = importance_mask(s, keep_fraction=0.5)
    assert m.dtype == torch.bool and tuple(m.shape) == (6,)


def test_importance_mask_refuses_bad_arguments():
    from gs4d_train.pruning import importance_mask
    s = _scores()
    with pytest.raises(ValueError):
        importance_mask(s)
    for kf in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            importance_mask(s, keep_fraction=kf)
    with pytest.raises(ValueError):
        importance_mask(s, keep_fraction=0.5, by="opacity")


# ---- the references and scenes of the GPU tests ---------------------------------------------------------------------
def test_reference_sum_telescopes_to_the_alpha_image(oracle):
    """sum_i sum_i = sum_p sum_i w_ip = sum_p (1 - Tfinal_p): T_{k+1} = T_k (1 - alpha_k), so alpha_k T_k =
    T_k - T_{k+1} and a pixel's weights telescope"""
    ref = DS.reference(oracle, "small0")
    sc = IR.reference_scores(DS.scene("small0")["s"], ref["export"]["point_list"], ref["export"]["ranges"])
    total, want = float(sc["sum"].sum()), float((1 - sc["Tfinal"]).sum())
    assert want > 10 and abs(total - want) <= 1e-12 * want
    # the restatement's Tfinal here is forward_autograd's, and its counts are n_contrib's slots
    assert torch.equal(sc["Tfinal"], ref["ref"]["Tfinal"].detach())
    assert int(sc["count"].sum()) > 0 and bool((sc["max"] <= 0.99).all()) and bool((sc["max"] >= 0).all())
    assert bool(((sc["count"] == 0) == (sc["sum"] == 0)).all())
    assert bool((sc["max"][sc["count"] > 0] >= 1 / 255).all())


def test_stack_scene_has_the_run_lengths_it_claims(oracle):
    s = IR.stack_scene()
    nr, color, depth, radii, st = o_forward(oracle, s)
    ex = st.export()
    T = s["gx"] * s["gy"]
    assert (s["gx"], s["gy"], s["W"], s["H"]) == (5, 2, 80, 32)
    assert nr == sum(IR.STACK_LENGTHS) and np.array_equal(radii, np.full(nr, 5))
    assert np.array_equal(ex["tiles_touched"], np.ones(nr, np.uint32))  # one tile per Gaussian
    r = np.asarray(ex["ranges"], np.int64)
    assert np.array_equal(r[:, 1] - r[:, 0], np.asarray(IR.STACK_LENGTHS))  # exact run lengths, tile by tile
    want_ranges, want_gid = TL.lexsort_lists(s["tile_of"], s["z"], T)
    assert np.array_equal(r, want_ranges) and np.array_equal(ex["point_list"], want_gid)
    # depth ties exist inside the long runs (the order there is by id)
    z = s["z"][s["tile_of"] == 9]
    assert len(np.unique(z)) < len(z)
    # the longest run's centre pixels terminate: fewer contributors than the list is long, T_final near 1e-4
    n_contrib, final_T = np.asarray(ex["n_contrib"]).reshape(32, 80), np.asarray(ex["final_T"]).reshape(32, 80)
    cy, cx = 16 + 8, 16 * 4 + 8
    assert 0 < n_contrib[cy, cx] < 513 and final_T[cy, cx] < 2e-4
    assert n_contrib[16 + 8, 16 * 2 + 8] == 256 and final_T[16 + 8, 16 * 2 + 8] > 1e-4  # tile 7's 256 run does not


def test_wide_scene_has_one_gaussian_over_most_tiles(oracle):
    s = IR.wide_scene()
    nr, color, depth, radii, st = o_forward(oracle, s)
    ex = st.export()
    assert s["means3D"].shape[0] == 21 and (s["W"], s["H"]) == (256, 256)
    assert int(ex["tiles_touched"][IR.WIDE_BIG]) == 256  # its 3-sigma rectangle is the whole grid
    # pairs of the large Gaussian whose half tiles hold a pixel with alpha >= 1/255: more than two waves of slots
    ref = TL.reach_reference(s, ex)
    mine = ref["gid"] == IR.WIDE_BIG
    assert int((ref["need"][mine] != 0).sum()) > 128
    assert s["means3D"][IR.WIDE_BIG, 2] > s["means3D"][np.arange(21) != IR.WIDE_BIG, 2].max()  # behind the others
