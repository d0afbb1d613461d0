"""CPU preconditions of tests/test_hexplane_paths_gpu.py: what its scenes (tests/hexplane_path_scenes.py) must be for
the bitwise GPU comparisons to mean something -- exact in fp32, and aimed at every route of the backward -- asserted
here so that a later edit to a builder, or a kernel change that moves the thresholds, cannot make the GPU test vacuous.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import hexplane_path_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")


def test_backward_plan_is_a_host_query():
    """_C.hexplane_backward_plan runs without a device, answers every F the layout admits and refuses the others."""
    from gs4d_train import _C
    for F in (4, 8, 16, 32, 64, 128, 256):
        npw, wcap = _C.hexplane_backward_plan(F)
        assert 1 <= npw <= 256 and npw * F <= 2048 and wcap >= 16, (F, npw, wcap)
        assert 256 % (F // 4) == 0 and npw % (256 // (F // 4)) == 0  # whole chunks of the workgroup's lanes
    assert _C.hexplane_backward_plan(256)[0] * (256 // 4) // 64 == _C.hexplane_backward_plan(256)[0]  # a point per wave
    for F in (0, 2, 12, 24, 260, 512):
        with pytest.raises(RuntimeError):
            _C.hexplane_backward_plan(F)


def test_layout_limits():
    """gs4d_hexplane_layout_init: sides up to 65535 (anchors pack as two unsigned 16-bit halves), at most 2^31 - 1
    cells per plane (cell indices are ints)."""
    L = ctypes.CDLL(LIB)
    lay = ctypes.create_string_buffer(1 << 12)
    six = ctypes.c_int * 6

    def init(W, H, F=4):
        return L.gs4d_hexplane_layout_init(lay, 1, F, six(*([3] * 5 + [W])), six(*([3] * 5 + [H])))

    assert init(3, 65535) == 0 and init(65535, 3) == 0 and init(32768, 65535) == 0
    assert init(3, 65536) != 0 and init(65536, 3) != 0 and init(0, 3) != 0
    assert init(32769, 65535) != 0 and init(65535, 65535) != 0


@pytest.mark.parametrize("name", S.EXACT)
def test_exact_scene_is_exact(name):
    """The fp32 torch graph equals the fp64 graph bitwise (features, dpts, every plane gradient), every fp64 value
    survives a round trip through fp32, every plane size is 2^k + 1 and no cell anchors more than 256 points."""
    s = S.scene(name)
    for W, H in s["sizes"]:
        assert (W - 1) & (W - 2) == 0 and (H - 1) & (H - 2) == 0 and W >= 2 and H >= 2
    assert S.max_points_per_cell(s["pts"], s["sizes"]) <= S.MAX_PER_CELL
    assert set(np.unique(np.concatenate([p.ravel() for p in s["planes"]]))) <= {0.0, 0.5, 1.0, 2.0}
    assert np.array_equal(s["dfeat"], np.rint(s["dfeat"])) and np.abs(s["dfeat"]).max() <= 3
    f32, d32, g32 = S.torch_graph(s, torch.float32)
    f64, d64, g64 = S.reference64(name)
    for a, b in zip([f32, d32] + g32, [f64, d64] + g64):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(b.float().double(), b)  # representable
        assert torch.equal(a.double(), b)          # and what fp32 arithmetic gives
    assert all(g.abs().max() > 0 for g in g64) or name == "zero_plane"
    assert (f64.abs().max() > 0 and d64.abs().max() > 0) or name == "zero_plane"  # (zero features, zero dpts)


def test_exact_scenes_clip_and_offset_rows():
    """Over the scene list: rows at 1.25, -1.5, exactly +1 and -1, rows half a cell off in each axis, rows on nodes."""
    pts = np.concatenate([S.scene(n)["pts"] for n in S.EXACT])
    for v in S.CLIPS:
        assert (pts == v).any(), v
    s = S.scene("short_last")
    D = S.coarse_cells(s["resos"])
    h = (s["pts"].astype(np.float64) + 1.0) * D
    inside = np.abs(s["pts"]) <= 1
    odd = inside & (np.rint(h) == h) & (np.rint(h) % 2 == 1)
    assert odd.any(0).all() and (odd.sum(1) <= 1).all() and (odd.sum(1) == 0).any()


def _records(name):
    s = S.scene(name)
    npw, wcap = S.plan(s["F"])
    return s, npw, wcap, S.classify(s["pts"], s["order"], s["sizes"], s["F"], npw, wcap)


@pytest.mark.parametrize("F", S.LADDER_F)
def test_ladder_scene_hits_every_threshold(F):
    """For every fp of F's ladder, with T = window_words // fp: a (workgroup, plane) with nc == T in class fp and
    one with nc == T + 1 in the next class, one cell high; and the last plane of level 0 direct in a two-level field.
    A failure names the scene and the target to re-aim (ladder_scene builds them from the plan)."""
    s, npw, wcap, recs = _records("ladder_F%d" % F)
    assert len(s["resos"]) == 2 and len(s["pts"]) == 2 * len(S.ladder(F)) * npw
    by = {(r["group"], r["level"], r["plane"]): r for r in recs}
    for t in s["targets"]:
        r = by[(t["group"], t["level"], t["plane"])]
        assert (r["nc"], r["cls"]) == (t["nc"], t["cls"]), ("re-aim ladder_F%d" % F, t, r)
        if "edge" in t:
            assert r["ch"] == 1 and r["cw"] == t["nc"]
    edges = {t["edge"]: t["cls"] for t in s["targets"] if "edge" in t}
    names = [S.class_name(F, fp, False) for fp in S.ladder(F)] + ["direct"]
    for i, fp in enumerate(S.ladder(F)):
        assert edges[(fp, 0)] == names[i] and edges[(fp, 1)] == names[i + 1]
        assert any(r["nc"] == wcap // fp and r["cls"] == names[i] for r in recs)
        assert any(r["nc"] == wcap // fp + 1 and r["cls"] == names[i + 1] for r in recs)
    assert {r["cls"] for r in recs} == set(names)  # every class of the ladder
    assert all(r["cls"] == "direct" for r in recs if (r["level"], r["plane"]) == (0, 5))  # then level 1 follows


@pytest.mark.parametrize("F", S.WIDE_F)
def test_wide_scene_has_a_full_a_sliced_and_a_direct_plane(F):
    s, npw, wcap, recs = _records("wide_F%d" % F)
    cls = {r["cls"] for r in recs}
    assert "full" in cls and "direct" in cls and any(c.startswith("slice") for c in cls), ("re-aim wide_F%d" % F, cls)
    assert all(r["cls"] == "full" and r["nc"] <= 4 for r in recs if r["group"] == 0)
    if F == 256:
        assert npw * (F // 4) == 8 * 64  # one point per wave


def test_edge_scenes_are_what_they_claim():
    """short_last, single, one_cell, corner, zero_plane, four_levels, the tall planes."""
    s, npw, _, recs = _records("short_last")
    assert len(s["pts"]) == npw + 1 and max(r["group"] for r in recs) == 1
    assert len(S.scene("single")["pts"]) == 1
    s, npw, _, recs = _records("one_cell")
    # one anchor where the plane's axes are the coarsest of their kind (half a coarse cell is a whole fine one)
    assert all(r["cls"] == "full" and r["cw"] <= 4 and r["ch"] <= 4 for r in recs if r["group"] == 0)
    assert [r["nc"] for r in recs if (r["group"], r["level"], r["plane"]) == (0, 1, 1)] == [4]
    assert len(np.unique(s["pts"][:npw], axis=0)) > 1
    s = S.scene("corner")
    last = s["pts"] >= 1
    assert (last.sum(1) >= 2).all() and (last.sum(1) == 4).any() and (s["pts"] == 1.25).any()
    for pg, (W, H) in enumerate(s["sizes"]):  # anchors on the last row and column of every plane: one tap inside
        c0, c1 = S.PAIRS[pg % 6]
        assert ((S.anchors(s["pts"][:, c0], W) == W - 1) & (S.anchors(s["pts"][:, c1], H) == H - 1)).any()
    s = S.scene("zero_plane")
    assert [int(np.abs(p).max() == 0) for p in s["planes"]] == [int(i == s["zero_plane"]) for i in range(12)]
    g = S.reference64("zero_plane")[2]
    assert [bool(x.any()) for x in g] == [i == s["zero_plane"] for i in range(12)]
    assert len(S.scene("four_levels")["sizes"]) == 24 and S.scene("four_levels")["F"] == 32
    for name, H in (("tall_exact", 32769), (S.TALL_40000, 40000)):
        s, npw, _, recs = _records(name)
        assert s["sizes"][2] == (3, H) and s["F"] == 4
        rows = S.anchors(s["pts"][:, 3], H)
        for r in s["rows"]:
            assert (rows[:npw] == r).any() or r > 32769
            assert (rows[npw:] == r).any()
        assert {r["cls"] for r in recs if r["plane"] == 2} == {"full", "direct"}
    # the 40000-row plane cannot be exact (tall_scene); its times leave the row coordinate within 2^-18 of a cell of
    # its exact value, so that a bilinear sample (1 - f) a + f b of values in {1/2, 1, 2} at f in [0.05, 0.95] moves
    # by at most 2^-18 |a - b| / min v <= 2^-18 * 1.5 / 0.575 = 1e-5 * 0.995 relative: inside the feature bar
    assert S.scene(S.TALL_40000)["row_err"] <= 2.0 ** -18


def test_general_scenes_keep_their_groups_boxes():
    """general(name): the same workgroups, every point inside its workgroup's box of the exact scene."""
    for name in S.EXACT:
        s, g = S.scene(name), S.general(name)
        npw, _ = S.plan(s["F"])
        assert g["pts"].shape == s["pts"].shape and g["pts"].dtype == np.float32
        for k in range(0, len(s["pts"]), npw):
            a, b = s["pts"][k:k + npw], g["pts"][k:k + npw]
            assert (b >= a.min(0)).all() and (b <= a.max(0)).all()
        assert all(0.1 <= p.min() and p.max() <= 1.2 for p in g["planes"])


def test_classifier_and_morton_restatement_on_known_cases():
    """The classifier on hand-worked boxes and the Morton restatement on hand-worked codes."""
    # F = 16, a 9 x 9 plane 0: two points at nodes (2, 3) and (5, 7) -> anchors box 4 x 5, touched 5 x 6 = 30 cells
    pts = np.array([[-0.5, -0.25, -1, -1], [0.25, 0.75, -1, -1]], np.float32)
    sizes = [(9, 9)] * 6
    r = S.classify(pts, [0, 1], sizes, 16, 128, 479)[0]
    assert (r["cw"], r["ch"], r["nc"], r["fp"], r["cls"]) == (5, 6, 30, 8, "slice 8")  # 30 * 16 = 480 > 479
    assert S.classify(pts, [0, 1], sizes, 16, 128, 480)[0]["cls"] == "full"
    assert S.classify(pts, [0, 1], sizes, 16, 128, 119)[0]["cls"] == "direct"  # 30 * 4 = 120 > 119
    assert S.classify(pts, [0, 1], sizes, 16, 128, 120)[0]["cls"] == "slice 4"
    r = S.classify(pts, [0, 1], sizes, 16, 1, 480)  # one point per workgroup: 2 x 2 boxes; on the last row, 2 x 1
    assert r[0]["nc"] == 4 and len(r) == 12
    edge = np.array([[1.0, 1.25, 0, 0]], np.float32)
    r = S.classify(edge, [0], sizes, 16, 1, 480)[0]
    assert (r["cw"], r["ch"]) == (1, 1)
    # Morton: x -> bit 0, y -> bit 1, z -> bit 2 of each octal digit, 8 bits per axis, clamped to 0 .. 255
    p = np.array([[-1, -1, -1, 0], [1, -1, -1, 0], [-1, 1.5, -1, 0], [-2, -1, 1, 0], [-1 + 1 / 128, -1, -1, 0],
                  [-1 + 2 / 128, -1 + 1 / 128, -1, 0]], np.float32)
    assert S.morton_codes(p).tolist() == [0, 0x249249, 0x492492, 0x924924, 1, 0b1010]
