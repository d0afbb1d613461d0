"""Scenes, references and a route classifier for the HexPlane field's backward (test infrastructure; importable
without a GPU).

hexplane.hip's backward sums every (point, tap, feature) term in 64-bit fixed point, and each (workgroup, level,
plane) takes one of several routes by the size of the workgroup's anchor box: an LDS window over all F features
(`full`), the same window in feature slices of F/2 ... 4 (`slice fp`), or direct global atomics (`direct`).  Two
properties make every route testable to the bit:

Exact arithmetic.  Integer sums are exact.  In an EXACT scene every term is exactly representable, so the fp32 torch
graph, the fp64 torch graph and the kernel must agree bitwise whatever the route, the summation order or the fmaf use:
    - every plane size is 2^k + 1, and per axis the coarsest level's cells (D[a]) divide every level's;
    - a coordinate is -1 + h / D[a] with h in half cells of that coarsest grid: a node of every level, at most one
      axis per point half a cell off (odd h), so every bilinear weight is 0, 1/2 or 1 and at most three of a
      level's six samples blend two values;
    - plane values are 1/2, 1 or 2 (a blend is k/4, k <= 8), dfeat is an integer in [-3, 3]: every term is a
      multiple of 2^-8 below 2^7 (2^-9 and 2^8 for the coordinate gradient);
    - at most 256 points land in one cell, so a cell's sum is a multiple of 2^-8 below 2^15: 23 bits;
    - some rows are clipped (1.25, -1.5, exactly +-1): a clipped coordinate sits on the border node.
test_hexplane_paths_boundary.py asserts the consequence on the CPU (fp32 graph == fp64 graph bitwise, every fp64 value
survives fp32) for every scene, so a later edit to a builder cannot make the GPU comparison approximate.

Caller-chosen grouping.  _C.hexplane_forward / _C.hexplane_backward take the point order, and a workgroup serves
points_per_workgroup consecutive points of it (_C.hexplane_backward_plan), so under order = arange the scene decides
which points share a workgroup: classify() restates the kernel's route rule per (workgroup, level, plane) from the
plan's two numbers -- never from copied constants -- and the boundary test asserts that every class and every
T / T + 1 edge (T = window_words // fp) is present.  Only coverage assertions use the classifier.

Scenes (EXACT, plus TALL_40000 which cannot be exact, see tall_scene):
    ladder_F{4,16,32}  two levels; for every fp of the ladder one workgroup whose plane 0 box has nc == T cells and
                       one with nc == T + 1 (anchors on the plane's last row, where the box is one cell high); the
                       (z, t) plane of level 0 -- the last plane before the next level's reverse pass overwrites
                       the LDS arrays -- is direct in every workgroup.
    short_last         N = points_per_workgroup + 1        single    N = 1
    one_cell           a workgroup whose points share one cell
    corner             anchors on last rows and columns (one tap inside), all four axes included
    zero_plane         one all-zero plane and a zero dfeat for the other level: eleven zero gradients, one nonzero
    wide_F{8,64,128,256}  one workgroup in one cell (full), corner-to-corner workgroups (sliced and direct planes)
    four_levels        GS4D_HEXPLANE_MAX_LEVELS levels at F = 32
    tall_exact         time planes of 32769 rows: anchors at rows 32767 and 32768 (y0 << 16 needs bit 31)
"""
import functools
import itertools

import numpy as np

PAIRS = list(itertools.combinations(range(4), 2))  # (c0, c1) of plane p: W = reso[c0], H = reso[c1]
VALUES = np.array([0.5, 1.0, 2.0], np.float32)
CLIPS = np.array([1.25, -1.5, 1.0, -1.0], np.float32)
MAX_PER_CELL = 256


@functools.lru_cache(maxsize=None)
def plan(F):
    """(points per workgroup, window words) of the backward at F features, from the library."""
    from gs4d_train import _C
    npw, wcap = _C.hexplane_backward_plan(F)
    return int(npw), int(wcap)


def ladder(F):
    """the features per pass the kernel tries, in order"""
    out, fp = [], F
    while fp >= 4:
        out.append(fp)
        fp //= 2
    return out


def class_name(F, fp, direct):
    return "direct" if direct else ("full" if fp == F else "slice %d" % fp)


# ---- the route rule -------------------------------------------------------------------------------------------------
def anchors(c, size):
    """make_tap's anchor index of coordinates c on an axis of `size` nodes, in fp32 as the kernel computes it
    (grid_sampler_unnormalize with align_corners, clipped to the border)"""
    c = np.asarray(c, np.float32)
    v = ((c + np.float32(1)) / np.float32(2)) * np.float32(size - 1)
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(size - 1))
    return np.floor(v).astype(np.int64)


def classify(pts, order, sizes, F, npw, wcap):
    """One record per (workgroup, level, plane): the anchor box, the touched cells cw x ch = nc, the features per pass
    fp and the class, as hexplane_backward_kernel decides them.  sizes: (W, H) of the 6 * levels planes."""
    pts = np.asarray(pts, np.float32)
    order = np.asarray(order, np.int64)
    out = []
    for g in range(-(-len(order) // npw)):
        rows = pts[order[g * npw:(g + 1) * npw]]
        for pg, (W, H) in enumerate(sizes):
            c0, c1 = PAIRS[pg % 6]
            x0, y0 = anchors(rows[:, c0], W), anchors(rows[:, c1], H)
            ax0, ay0 = int(x0.min()), int(y0.min())
            aw, ah = int(x0.max()) - ax0 + 1, int(y0.max()) - ay0 + 1
            cw = min(ax0 + aw, W - 1) - ax0 + 1  # the anchors' box and its +1 neighbours inside the plane
            ch = min(ay0 + ah, H - 1) - ay0 + 1
            nc, fp = cw * ch, F
            while nc * fp > wcap and fp > 4:
                fp //= 2
            out.append(dict(group=g, level=pg // 6, plane=pg % 6, cw=cw, ch=ch, nc=nc, fp=fp,
                            cls=class_name(F, fp, nc * fp > wcap)))
    return out


def max_points_per_cell(pts, sizes):
    """the largest number of points anchored at one cell of one plane"""
    worst = 0
    for pg, (W, H) in enumerate(sizes):
        c0, c1 = PAIRS[pg % 6]
        cell = anchors(pts[:, c1], H) * W + anchors(pts[:, c0], W)
        worst = max(worst, int(np.unique(cell, return_counts=True)[1].max()))
    return worst


# ---- the Morton order -----------------------------------------------------------------------------------------------
def morton_codes(pts):
    """hex_morton_kernel's 24-bit codes (quant8 / spread3 of x, y, z) in numpy fp32"""
    def quant8(c):
        v = (np.asarray(c, np.float32) + np.float32(1)) * np.float32(128)
        q = np.where(v > 0, np.minimum(v, np.float32(255)), np.float32(0))  # NaN -> 0
        return np.floor(q).astype(np.uint32)

    def spread3(x):
        x = x.astype(np.uint32)
        x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
        x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
        x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
        x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
        return x

    return (spread3(quant8(pts[:, 0])) | (spread3(quant8(pts[:, 1])) << np.uint32(1))
            | (spread3(quant8(pts[:, 2])) << np.uint32(2)))


def morton_order(pts):
    return np.argsort(morton_codes(pts), kind="stable")


# ---- exact scenes ---------------------------------------------------------------------------------------------------
def sizes_of(resos):
    return [(r[c0], r[c1]) for r in resos for c0, c1 in PAIRS]


def coarse_cells(resos):
    D = [min(r[a] - 1 for r in resos) for a in range(4)]
    for r in resos:
        for a in range(4):
            n = r[a] - 1
            assert n >= 1 and n & (n - 1) == 0 and n % D[a] == 0, resos  # 2^k + 1 nodes, nested grids
    return np.array(D, np.int64)


def rand_group(rng, n, D, lo=None, hi=None, span=True, clip_axes=(0, 1, 2, 3), clip_share=0.12):
    """n points on the nodes lo .. hi (coarse cells per axis, default the whole field), at most one axis per point
    half a cell up; span: point 0 sits on lo and point 1 on hi, so the group's anchor box is exactly lo .. hi.
    Returns the half-cell numerators h (n, 4) and the clipped overrides (n, 4; NaN: none), which only ever
    replace a coordinate of a point that keeps the group's box (never points 0 and 1)."""
    lo = np.zeros(4, np.int64) if lo is None else np.asarray(lo, np.int64)
    hi = D.copy() if hi is None else np.asarray(hi, np.int64)
    j = rng.integers(lo, hi + 1, (n, 4))
    if span and n >= 2:
        j[0], j[1] = lo, hi
    h = 2 * j
    ax = rng.integers(-1, 4, n)
    for i in range(2 if span else 0, n):
        if ax[i] >= 0 and j[i, ax[i]] < hi[ax[i]]:
            h[i, ax[i]] += 1
    clip = np.full((n, 4), np.nan, np.float32)
    if clip_axes:
        for i in range(2 if span else 0, n):
            if rng.random() < clip_share:
                a = int(rng.choice(clip_axes))
                v = CLIPS[rng.integers(0, 4)]
                # a clipped coordinate sits on the border node: only where that node is inside the group's box
                if (v > 0 and hi[a] == D[a]) or (v < 0 and lo[a] == 0):
                    clip[i, a] = v
    return h, clip


def assemble(name, F, resos, parts, seed, zero_plane=None, zero_levels=()):
    """the scene dict from the groups' (h, clip) parts"""
    rng = np.random.default_rng(seed)
    D = coarse_cells(resos)
    h = np.concatenate([p[0] for p in parts])
    clip = np.concatenate([p[1] for p in parts])
    assert ((h % 2).sum(1) <= 1).all() and (h >= 0).all() and (h <= 2 * D).all()
    pts = (h.astype(np.float64) / D - 1.0).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), h.astype(np.float64) / D - 1.0)  # exactly representable
    pts = np.where(np.isnan(clip), pts, clip).astype(np.float32)
    sizes = sizes_of(resos)
    planes = [rng.choice(VALUES, (1, F, H, W)).astype(np.float32) for W, H in sizes]
    if zero_plane is not None:
        planes[zero_plane][:] = 0
    dfeat = rng.integers(-3, 4, (len(pts), len(resos) * F)).astype(np.float32)
    for l in zero_levels:
        dfeat[:, l * F:(l + 1) * F] = 0
    return dict(name=name, F=F, resos=[tuple(r) for r in resos], sizes=sizes, pts=pts, planes=planes, dfeat=dfeat,
                order=np.arange(len(pts)), targets=[])


def wide_axis_nodes(wcap):
    """the smallest 2^k + 1 that holds a one-row box of window_words // 4 + 1 cells off the last column"""
    n = 4
    while n < wcap // 4 + 2:
        n *= 2
    return n + 1


def ladder_scene(F):
    npw, wcap = plan(F)
    rng = np.random.default_rng(100 + F)
    Wx = wide_axis_nodes(wcap)
    resos = [(Wx, 3, 33, 65), (Wx, 5, 9, 9)]
    D = coarse_cells(resos)
    parts, targets = [], []
    for fp in ladder(F):
        T = wcap // fp
        assert T >= 2
        for nc in (T, T + 1):
            # anchors a .. a + nc - 2 on the last row of plane 0 (y = +1): cw = nc, ch = 1
            a = int(rng.integers(0, D[0] - nc + 2))
            lo, hi = np.array([a, D[1], 0, 0]), np.array([a + nc - 2, D[1], D[2], D[3]])
            h, clip = rand_group(rng, npw, D, lo, hi, clip_axes=(1, 2, 3))
            nxt = fp // 2
            cls = class_name(F, fp, False) if nc == T else class_name(F, nxt, nxt < 4)
            for level in (0, 1):
                targets.append(dict(group=len(parts), level=level, plane=0, nc=nc, cls=cls, edge=(fp, nc - T)))
            # (z, t) of level 0 spans the plane: direct, then level 1 reuses the LDS arrays
            targets.append(dict(group=len(parts), level=0, plane=5, nc=resos[0][2] * resos[0][3], cls="direct"))
            parts.append((h, clip))
    s = assemble("ladder_F%d" % F, F, resos, parts, 200 + F)
    s["targets"] = targets
    return s


SMALL = [(9, 5, 9, 17), (5, 9, 3, 5)]


def misc_scene(name):
    F = 16
    npw, _ = plan(F)
    rng = np.random.default_rng(sum(map(ord, name)))
    resos = SMALL
    D = coarse_cells(resos)
    zero_plane, zero_levels = None, ()
    if name == "short_last":
        parts = [rand_group(rng, npw, D), rand_group(rng, 1, D, span=False)]
    elif name == "single":
        parts = [rand_group(rng, 1, D, span=False, clip_axes=())]
    elif name == "one_cell":
        j = np.array([1, 2, 0, 3])
        parts = [rand_group(rng, npw, D, j, j + 1, span=False, clip_axes=()), rand_group(rng, 5, D)]
        parts[0][0][:] = 2 * j + (parts[0][0] % 2)  # every point on node j, at most one axis half a cell up
    elif name == "corner":
        h, clip = rand_group(rng, npw + 9, D, clip_axes=())
        for i in range(len(h)):
            axes = rng.permutation(4)[:rng.integers(2, 5)]
            if i == 2:
                axes = np.arange(4)
            h[i, axes] = 2 * D[axes]  # the last node of two to four axes
            if i % 3 == 0:
                clip[i, axes[0]] = 1.25
        parts = [(h, clip)]
    elif name == "zero_plane":
        parts = [rand_group(rng, npw, D), rand_group(rng, npw // 2 + 3, D)]
        zero_plane, zero_levels = 3, (1,)
    else:
        raise KeyError(name)
    s = assemble(name, F, resos, parts, 300 + len(name), zero_plane, zero_levels)
    s["zero_plane"] = zero_plane
    return s


def wide_scene(F):
    npw, _ = plan(F)
    rng = np.random.default_rng(400 + F)
    resos = [(9, 5, 33, 129)]
    D = coarse_cells(resos)
    j = np.array([3, 1, 17, 60])
    one = rand_group(rng, npw, D, j, j + 1, span=False, clip_axes=())
    one[0][:] = 2 * j + (one[0] % 2)
    parts = [one, rand_group(rng, npw, D), rand_group(rng, npw, D), rand_group(rng, 1, D, span=False)]
    s = assemble("wide_F%d" % F, F, resos, parts, 500 + F)
    s["classes"] = ["full", "slice", "direct"]
    return s


def four_level_scene():
    F = 32
    npw, _ = plan(F)
    rng = np.random.default_rng(77)
    resos = [(9, 5, 9, 17), (17, 9, 17, 17), (5, 5, 9, 33), (9, 9, 5, 17)]
    D = coarse_cells(resos)
    parts = [rand_group(rng, npw, D), rand_group(rng, npw, D, [1, 1, 0, 4], [2, 3, 2, 9]),
             rand_group(rng, npw, D), rand_group(rng, 5, D)]
    return assemble("four_levels", F, resos, parts, 78)


def tall_scene(exact):
    """Time planes with rows past 32767, F = 4.  Workgroup 0 keeps its times at the rows around 32768 (a window route),
    workgroup 1 spreads them over the whole axis (direct).

    exact: 32769 rows (2^15 + 1).  Anchors at row 32766, 32767 (on the node, and half a cell up: taps on 32767 and
    32768) and 32768 (the border row).
    not exact (TALL_40000): the (x, t) plane alone has 40000 rows, anchors at rows 32767, 32768 and 39998.  No exact
    scene exists there: the row coordinate is ((t + 1) / 2) * 39999 with 39999 odd and t + 1 = n 2^-23, so the product
    n 39999 2^-24 is a multiple of the fp32 spacing at rows >= 32768 (2^-8) only when 2^16 divides n, i.e. at rows
    k 39999 / 256 -- none within a cell of the three.  fp32 (the kernel and torch alike) then rounds the row
    coordinate by up to 2^-9 of a cell, which is no error of the kernel.  Each time is searched among the floats of
    its row for the one whose fp32 row coordinate is nearest its exact value (row_err: the worst distance, in
    cells), and the scene is compared under the general-value bars, which row_err must leave room for (the
    boundary test asserts it)."""
    F = 4
    npw, _ = plan(F)
    rng = np.random.default_rng(9 if exact else 10)
    if exact:
        resos = [(3, 3, 3, 32769)]
        D = coarse_cells(resos)
        near = rand_group(rng, npw, D, [0, 0, 0, 32766], [2, 2, 2, 32768], clip_axes=(0, 1, 2))
        far = rand_group(rng, 40, D, clip_axes=(0, 1, 2))
        far[0][2:8, 3] = 2 * np.array([32767, 32768, 16384, 32766, 32767, 1]) + np.array([1, 0, 0, 1, 0, 0])
        far[0][2:8, :3] -= far[0][2:8, :3] % 2
        s = assemble("tall_exact", F, resos, [near, far], 11)
        s["rows"] = [32767, 32768]
        return s
    resos = [(3, 3, 3, 5)]
    D = coarse_cells(resos)
    s = assemble("tall_40000", F, resos, [rand_group(rng, npw, D, clip_axes=()), rand_group(rng, 40, D, clip_axes=())], 12)
    H = 40000
    s["sizes"][2] = (3, H)
    s["planes"][2] = rng.choice(VALUES, (1, F, H, 3)).astype(np.float32)
    near = [(r, 0.05, 0.95) for r in (32766, 32767, 32768, 32769)]
    far = [(r, 0.05, 0.95) for r in (0, 16384, 32767, 32768, 39998)] + [(39999, 0.0, 0.0)]
    times = {w: _tall_time(w, H) for w in near + far}
    pick = [near[i] for i in rng.integers(0, len(near), npw)] + [far[i % len(far)] for i in range(40)]
    s["pts"][:, 3] = np.array([times[w][0] for w in pick], np.float32)
    s["row_err"] = max(e for _, e in times.values())
    s["rows"] = [32767, 32768, 39998]
    return s


def _tall_time(want, H):
    """(t, |fp32 row coordinate - exact|) of the float t in row want[0], at a fraction within want[1:], whose fp32
    row coordinate (make_tap's arithmetic) is nearest its exact value"""
    row, f_lo, f_hi = want
    if row == H - 1:
        return np.float32(1.0), 0.0
    c = np.float32(2.0 * (row + f_lo) / (H - 1) - 1.0)
    cand = [c]
    while len(cand) < 4000 and (float(cand[-1]) + 1.0) / 2.0 * (H - 1) < row + f_hi:
        cand.append(np.nextafter(cand[-1], np.float32(2)))
    cand = np.array(cand, np.float32)
    v32 = ((cand + np.float32(1)) / np.float32(2)) * np.float32(H - 1)
    v64 = (cand.astype(np.float64) + 1.0) / 2.0 * (H - 1)  # exact in fp64: 25 + 16 bits
    err = np.where(np.floor(v64) == row, np.abs(v32.astype(np.float64) - v64), np.inf)
    i = int(np.argmin(err))
    return cand[i], float(err[i])


LADDER_F = (4, 16, 32)
WIDE_F = (8, 64, 128, 256)
MISC = ("short_last", "single", "one_cell", "corner", "zero_plane")
EXACT = (["ladder_F%d" % F for F in LADDER_F] + list(MISC) + ["wide_F%d" % F for F in WIDE_F]
         + ["four_levels", "tall_exact"])
TALL_40000 = "tall_40000"
ALL = EXACT + [TALL_40000]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("ladder_F"):
        return ladder_scene(int(name[8:]))
    if name.startswith("wide_F"):
        return wide_scene(int(name[6:]))
    if name == "four_levels":
        return four_level_scene()
    if name.startswith("tall_"):
        return tall_scene(name == "tall_exact")
    return misc_scene(name)


def general(name, lattice=True):
    """the scene's group layout with general values: planes uniform in [0.1, 1.2], every point uniform inside its
    workgroup's coordinate box, randn dfeat.

    lattice (default): the uniform draw is rounded to multiples of 2^-20 (1024 positions per cell of the widest axis
    here, 32 on the 32769-row one).  On an axis of 2^k + 1 nodes fp32 then unnormalises the coordinate exactly --
    c + 1, / 2 and * 2^k are all exact -- as fp64 does.  Without it the comparison measures fp32's coordinate
    rounding, not the kernel: on the 2049-node axis the row coordinate is rounded to 2^-13 of a cell, and the fp32
    torch graph itself then misses the feature bar by the same factor as the kernel, digit for digit (measured on
    the unrounded draw, kernel = fp32 graph: ladder_F4 12.0, ladder_F16 6.6, ladder_F32 9.0, tall_exact 318 times
    the bar; general(name, lattice=False) reproduces the draw)."""
    return _general(name, bool(lattice))


@functools.lru_cache(maxsize=None)
def _general(name, lattice):
    s = scene(name)
    npw, _ = plan(s["F"])
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    pts = s["pts"].copy()
    for g in range(-(-len(pts) // npw)):
        rows = s["pts"][g * npw:(g + 1) * npw]
        lo, hi = rows.min(0), rows.max(0)  # (multiples of 2^-15: rounding to the lattice stays inside)
        u = rng.uniform(lo, hi, rows.shape)
        pts[g * npw:(g + 1) * npw] = (np.rint(u * 2.0 ** 20) / 2.0 ** 20 if lattice else u).astype(np.float32)
    planes = [rng.uniform(0.1, 1.2, p.shape).astype(np.float32) for p in s["planes"]]
    dfeat = rng.standard_normal(s["dfeat"].shape).astype(np.float32)
    return dict(s, pts=pts, planes=planes, dfeat=dfeat)


# ---- references -----------------------------------------------------------------------------------------------------
def torch_graph(s, dtype):
    """(feat, dpts, plane gradients) of interpolate_ms_features' grid_sample graph on the CPU in `dtype`"""
    import torch

    from gs4d_train.deformation import interpolate_ms_features
    pts = torch.tensor(s["pts"], dtype=dtype, requires_grad=True)
    planes = [torch.tensor(p, dtype=dtype, requires_grad=True) for p in s["planes"]]
    feat = interpolate_ms_features(pts, [planes[i:i + 6] for i in range(0, len(planes), 6)])
    g = torch.autograd.grad(feat, [pts] + planes, torch.tensor(s["dfeat"], dtype=dtype))
    return feat.detach(), g[0], list(g[1:])


@functools.lru_cache(maxsize=None)
def reference64(name, kind="exact"):
    """the fp64 graph of scene(name) (kind exact) or general(name); computed once, shared, never modified"""
    import torch
    return torch_graph(scene(name) if kind == "exact" else general(name), torch.float64)
