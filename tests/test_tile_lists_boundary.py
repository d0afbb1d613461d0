"""CPU preconditions of tests/test_tile_lists_gpu.py: what its scenes (tests/tile_list_scenes.py) must be for the
exact GPU comparisons to mean something, asserted against the oracle so that a later edit to a builder cannot make
the GPU test vacuous -- and the list checkers themselves, on the oracle's own lists and on corrupted copies.
"""
import numpy as np
import pytest

import tile_list_scenes as TL
from gpu_helpers import o_bounds
from gs4d_train.synthetic import make_upstream_grad
from oracle import parity as PAR


def _oracle_lists(ex, s):
    """the oracle's lists in gs4d_debug_tile_lists' form (every pair emitted, both bits, slot = candidate number)"""
    n = len(ex["point_list"])
    gid = np.asarray(ex["point_list"], np.int64)
    r = np.asarray(ex["ranges"], np.int64)
    order = np.argsort(-np.minimum(r[:, 1] - r[:, 0], 1023), kind="stable")
    # emission order: Gaussians in id order; here every Gaussian has one tile, so slot = rank of the id
    slot = np.argsort(np.argsort(gid, kind="stable"), kind="stable")
    return dict(ranges=r, order=order, n=n, gid=gid, reach=np.full(n, 3, np.uint8), slot=slot,
                depth=np.asarray(ex["depths"], np.float32)[gid])


@pytest.mark.parametrize("name", TL.ORACLE_STACKS + list(TL.TOTALS))
def test_stack_scene_is_what_the_gpu_test_assumes(oracle, name):
    s = TL.scene(name)["s"]
    run = TL.oracle_run(oracle, name)
    ex = run["export"]
    P, T = len(s["means3D"]), s["gx"] * s["gy"]
    vis = s["tile_of"] >= 0
    assert run["nr"] == int(vis.sum()) == int(s["lengths_by_tile"].sum())
    assert np.array_equal(run["radii"][vis], np.full(int(vis.sum()), 5)) and not run["radii"][~vis].any()
    if run["nr"]:
        assert np.array_equal(ex["tiles_touched"][vis], np.ones(int(vis.sum()), np.uint32))  # one tile per Gaussian
        assert np.array_equal(TL.depth_bits(ex["depths"])[vis], TL.depth_bits(s["z"])[vis])  # view depth = z, bitwise
    r = np.asarray(ex["ranges"], np.int64)
    assert np.array_equal(r[:, 1] - r[:, 0], s["lengths_by_tile"])  # exact run lengths
    want_ranges, want_gid = TL.lexsort_lists(s["tile_of"], s["z"], T)
    assert np.array_equal(r, want_ranges) and np.array_equal(ex["point_list"], want_gid)
    if name.startswith("7x4") or name.startswith("32x9"):
        assert sorted(s["lengths_by_tile"][s["lengths_by_tile"] > 0]) == sorted(x for x in TL.LENGTHS if x)
        # both halves of every pair are reachable, so the GPU's reach must be 3 everywhere
        ref = TL.reach_of(oracle, name)
        assert np.array_equal(ref["need"], np.full(run["nr"], 3, np.uint8)) and not ref["nonpd"].any()
        # the flagged shares stay inside oracle/parity.py's defaults (the consumers' test uses check() as it is)
        g = make_upstream_grad(run["color"])[0] * (3 * s["W"] * s["H"])
        b = o_bounds(oracle, s, run["state"], run["radii"], g)
        assert (np.asarray(b["pflag"]) != 0).mean() <= PAR.FLIP_PIX_FRAC
        assert (np.asarray(b["gflag"]) != 0).mean() <= PAR.FLIP_GAUSS_FRAC
    if run["nr"]:
        lists = _oracle_lists(ex, s)
        assert TL.structure_errors(lists, T, run["nr"], P) == []
        assert TL.order_errors(lists, s["z"]) == []
        assert TL.oracle_order_errors(lists, ex, P) == []


def test_the_large_grid_stack_takes_the_radix_binning():
    s = TL.scene("129x129_random")["s"]
    T = s["gx"] * s["gy"]
    assert T == 16641 > 16384 and s["W"] == s["H"] == 2064
    assert sorted(s["lengths_by_tile"][s["lengths_by_tile"] > 0]) == sorted(x for x in TL.LENGTHS if x)
    assert s["lengths_by_tile"][T - 1] > 0 and s["lengths_by_tile"][0] == 0


def test_total_scenes_land_on_the_chunk_sizes():
    assert [TL.scene(f"total_{n}")["s"]["means3D"].shape[0] for n in (2047, 2048, 2049, 8191, 8192, 8193, 16385)] == \
        [2047, 2048, 2049, 8191, 8192, 8193, 16385]
    for n in (1, 2, 1023, 1024, 1025, 2049):
        s = TL.scene(f"culled_{n}")["s"]
        assert len(s["means3D"]) == n
        vis = s["tile_of"] >= 0
        assert int((~vis).sum()) == (n + 2) // 3 and np.all(s["means3D"][~vis, 2] < 0.2)  # V != P


@pytest.mark.parametrize("name", list(TL.AUDITS))
def test_audit_scene_has_pairs_of_every_kind(oracle, name):
    sc = TL.scene(name)
    ex = TL.oracle_run(oracle, name)["export"]
    st = TL.reach_stats(TL.reach_of(oracle, name))
    print(f"[tile-lists] {name}: L = {st['pairs']}, reachable {st['reachable']}, unreachable {st['unreachable']}, "
          f"one half {st['one_half']}, not positive definite {st['nonpd']}, within 1e-4 of 1/255: {st['near']}")
    assert st["pairs"] == ex["L"] == TL.oracle_run(oracle, name)["nr"]
    assert np.array_equal(sc["s"]["viewmatrix"], np.eye(4, dtype=np.float32))
    assert np.array_equal(TL.depth_bits(ex["depths"])[np.unique(ex["point_list"])],
                          TL.depth_bits(sc["s"]["means3D"][:, 2])[np.unique(ex["point_list"])])
    if name in TL.GENERAL_AUDITS:
        assert st["reachable"] >= 500 and st["unreachable"] >= 500 and st["one_half"] >= 500
    if name == "giant":
        assert (ex["tiles_touched"][TL.GIANT_IDS] > 2048).all()
        assert ex["tiles_touched"][np.setdiff1d(np.arange(200), TL.GIANT_IDS)].max() < 2048
        s = sc["s"]
        # a rectangle width that is no power of two: the emission's row-major position needs a real division
        r = TL.oracle_run(oracle, name)["radii"][TL.GIANT_IDS].astype(np.float64)
        x = ex["means2D"][TL.GIANT_IDS, 0].astype(np.float64)
        w = np.minimum(64, np.maximum(0, ((x + r + 15) // 16))) - np.minimum(64, np.maximum(0, (x - r) // 16))
        assert any(int(v) & (int(v) - 1) for v in w), w
    if name == "indef_small":
        assert st["nonpd"] >= 10 and sc["cov3D"] is not None


def test_debug_entry_is_declared_exported_and_checks_its_arguments():
    import ctypes
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gs4d.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int gs4d_debug_tile_lists\s*\(([^;]*)\);", text, flags=re.S)
    assert m and "read-only" in m.group(1) and "num_rendered == 0" in m.group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")] == [
        "int P", "int width", "int height", "int num_rendered", "const char *geometry_buffer",
        "const char *binning_buffer", "const char *image_buffer", "uint32_t *ranges", "uint32_t *order",
        "uint32_t *n_emitted", "uint32_t *gid", "uint32_t *reach", "uint32_t *slot", "float *depth", "void *stream"]
    path = os.path.join(root, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
    if not os.path.exists(path):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    lib.gs4d_last_error.restype = ctypes.c_char_p
    null, i = ctypes.c_void_p(0), ctypes.c_int
    some = ctypes.cast((ctypes.c_float * 16)(), ctypes.c_void_p)
    ok = [i(4), i(16), i(16), i(3)] + [some] * 10 + [null]
    for k, bad in ((0, i(0)), (1, i(0)), (2, i(-1)), (3, i(-1)), (4, null), (5, null), (6, null), (7, null), (8, null),
                   (9, null), (10, null), (13, null)):
        args = list(ok)
        args[k] = bad
        assert lib.gs4d_debug_tile_lists(*args) == 1, k  # GS4D_ERR_ARG before anything is launched
        assert lib.gs4d_last_error().startswith(b"debug_tile_lists:")
    import diff_gaussian_rasterization as dgr
    assert hasattr(dgr._C, "debug_tile_lists")


def test_the_checkers_notice_a_wrong_list(oracle):
    """The oracle's own list passes; one swapped pair, one dropped reachable pair, one cleared bit do not."""
    name = "7x4_ties"
    s = TL.scene(name)["s"]
    run = TL.oracle_run(oracle, name)
    ex, P, T = run["export"], len(s["means3D"]), 28
    good = _oracle_lists(ex, s)
    ref = TL.reach_of(oracle, name)
    assert TL.culling_errors(good, ref, P)[0] == []
    swapped = {k: np.array(v, copy=True) for k, v in good.items()}
    i = int(good["ranges"][TL.LENGTHS.index(8193), 1]) - 2  # the last two entries of the longest list
    for k in ("gid", "slot", "depth"):
        swapped[k][[i, i + 1]] = swapped[k][[i + 1, i]]
    assert TL.order_errors(swapped, s["z"]) and TL.oracle_order_errors(swapped, ex, P)
    cleared = dict(good, reach=np.where(np.arange(good["n"]) == 5, 1, 3).astype(np.uint8))
    assert TL.culling_errors(cleared, ref, P)[0]
    t = TL.LENGTHS.index(513)
    keep = np.arange(good["n"]) != good["ranges"][t, 0]
    rr = good["ranges"].copy()
    rr[t, 1] -= 1
    rr[t + 1:][rr[t + 1:, 1] > 0] -= 1
    dropped = dict(good, ranges=rr, n=good["n"] - 1, **{k: good[k][keep] for k in ("gid", "reach", "slot", "depth")})
    assert TL.structure_errors(dropped, T, run["nr"], P) == []
    assert TL.culling_errors(dropped, ref, P)[0]
    twice = dict(good, gid=np.where(np.arange(good["n"]) == i, good["gid"][i + 1], good["gid"]))
    assert TL.structure_errors(twice, T, run["nr"], P)
