"""Scenes and exact references for the rasterizer's two discrete stages: the per-tile (depth bits, id) sort and the
exact tile culling (test infrastructure; importable without a GPU).

The parity tests compare images and gradients and forgive a share of near-threshold pixels and Gaussians; a wrong
list order deep in a long list (T < 1e-4 there) or an over-eager cull (alpha ~ 1/255) shows exactly where that
allowance forgives it.  Here the lists themselves (gs4d_debug_tile_lists) are compared, with no tolerance, against a
numpy lexsort, the oracle's point_list and an fp64 evaluation of the reference's alpha test.

Every scene uses make_scene's identity-view camera: a Gaussian's view depth is its z, bit for bit.

Stack scenes  stack_scene(lengths, gx, seed, depth_mode): listed tile t gets exactly lengths[t] Gaussians, centred at
              pixel (16 tx + 8, 16 ty + 8) +- 0.3 px, identity rotation, isotropic scale 1.2 z / focal_x (1.2 px;
              radius 5, so the 3-sigma rectangle is that one tile), opacity 0.03 (alpha >= 1/255 within ~2.6 px of
              the centre: both half tiles are reached), ids shuffled over the tiles.  LENGTHS holds the edges of the
              six sort paths (1 | 2-64 | 65-128 | 129-256 in render.hip, 257-2048 with 512 / 1024 / 2048 key spaces
              and > 2048 in binning.hip).  depth_mode: random, ties (z = k / 4), equal (the order is by id alone),
              sorted, reverse (z ascending / descending in the id).
Total scenes  stacks whose number of candidates lands on the emission chunk (2048), the counting chunk at 8 keys per
              lane (8192) and, with every third Gaussian behind the near plane, the visible scan's chunk (1024).
Audit scenes  general splats over many tiles, for the culling: four make_scene scenes, `giant` (a 64x48-tile image
              with splats whose rectangle holds more than 2048 tiles, so one Gaussian fills whole emission chunks,
              and rectangle widths that are no power of two) and rule_scenes' indef_small (conics that are not
              positive definite are never culled).
"""
import math

import numpy as np

from gs4d_train.synthetic import make_scene

LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095,
           4096, 4097, 6143, 6145, 8193, 3]
assert sum(LENGTHS) == 44871
DEPTH_MODES = ["random", "ties", "equal", "sorted", "reverse"]
OPACITY = 0.03
ALPHA_MIN = 1.0 / 255.0


def stack_scene(lengths, gx, seed, depth_mode, gy=None, tiles=None):
    """make_scene's dict (sh_degree 0) plus tile_of (P,): the tile of each Gaussian, lengths_by_tile (T,) and z."""
    lengths = np.asarray(lengths, np.int64)
    gy = -(-len(lengths) // gx) if gy is None else gy
    T = gx * gy
    tiles = np.arange(len(lengths)) if tiles is None else np.asarray(tiles, np.int64)
    assert len(tiles) == len(lengths) and len(np.unique(tiles)) == len(tiles) and tiles.max() < T
    P, W, H = int(lengths.sum()), 16 * gx, 16 * gy
    rng = np.random.default_rng(1000 + seed)
    s = make_scene(P, W, H, seed=seed, sh_degree=0)
    tile_of = rng.permutation(np.repeat(tiles, lengths))  # ids shuffled over the tiles
    if depth_mode == "random":
        z = rng.uniform(2.0, 10.0, P)
    elif depth_mode == "ties":
        z = rng.integers(8, 41, P) / 4.0
    elif depth_mode == "equal":
        z = np.full(P, 5.0)
    elif depth_mode in ("sorted", "reverse"):
        z = np.sort(rng.uniform(2.0, 10.0, P))
        z = z if depth_mode == "sorted" else z[::-1]
    else:
        raise ValueError(depth_mode)
    z = z.astype(np.float32)
    px = 16 * (tile_of % gx) + 8 + rng.uniform(-0.3, 0.3, P)
    py = 16 * (tile_of // gx) + 8 + rng.uniform(-0.3, 0.3, P)
    # ndc2Pix: pix = ((ndc + 1) S - 1) / 2, ndc = x / (z tan_fov)
    zd = z.astype(np.float64)
    x = ((2 * px + 1) / W - 1) * zd * s["tanfovx"]
    y = ((2 * py + 1) / H - 1) * zd * s["tanfovy"]
    focal_x = W / (2.0 * s["tanfovx"])
    s["means3D"] = np.stack([x, y, zd], 1).astype(np.float32)
    assert np.array_equal(s["means3D"][:, 2], z)
    s["scales"] = np.repeat((1.2 * zd / focal_x)[:, None], 3, 1).astype(np.float32)
    s["rotations"] = np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1))
    s["opacities"] = np.full((P, 1), OPACITY, np.float32)
    by_tile = np.zeros(T, np.int64)
    by_tile[tiles] = lengths
    s.update(tile_of=tile_of, lengths_by_tile=by_tile, z=z, gx=gx, gy=gy)
    return s


def spread_tiles(n, T):
    """n distinct tiles from the first to the last of T"""
    t = np.round(np.linspace(0, T - 1, n)).astype(np.int64)
    assert len(np.unique(t)) == n
    return t


# name -> builder.  7x4 tiles: one radix pass's worth of key bits (msb(28) = 5), the final ping-pong buffer is 1;
# 32x9: 288 tiles, two passes, final buffer 0, most tiles empty; 129x129: 16,641 tiles > kCountMaxT = 16384, the radix
# binning with no environment variable (three passes' worth of bits would need 2^16 tiles; this has two)
def _stack7x4(mode):
    return lambda: stack_scene(LENGTHS, 7, 40 + DEPTH_MODES.index(mode), mode)


STACKS = {f"7x4_{m}": _stack7x4(m) for m in DEPTH_MODES}
STACKS["32x9_random"] = lambda: stack_scene(LENGTHS, 32, 50, "random", gy=9, tiles=spread_tiles(len(LENGTHS), 288))
STACKS["32x9_ties"] = lambda: stack_scene(LENGTHS, 32, 51, "ties", gy=9, tiles=spread_tiles(len(LENGTHS), 288))
STACKS["129x129_random"] = lambda: stack_scene(LENGTHS, 129, 52, "random", gy=129,
                                               tiles=spread_tiles(len(LENGTHS), 129 * 129))
ORACLE_STACKS = [n for n in STACKS if not n.startswith("129")]  # the 2064x2064 case needs no oracle run


def _split3(n):
    return [n // 3, n // 3, n - 2 * (n // 3), 0]


def total_scene(P, seed, cull_third=False):
    """A 2x2-tile stack scene (three tiles used) of P Gaussians; cull_third: Gaussians 0, 3, 6, .. lie behind the near
    plane (z = 0.1), so the visible scan compacts V = P - ceil(P / 3) of P (P = 1: nothing is visible)."""
    vis = np.arange(P) % 3 != 0 if cull_third else np.ones(P, bool)
    V = int(vis.sum())
    st = stack_scene(_split3(V), 2, seed, "ties")
    if not cull_third:
        return st
    s = make_scene(P, st["W"], st["H"], seed=seed, sh_degree=0)
    s["means3D"] = np.tile(np.array([0, 0, 0.1], np.float32), (P, 1))
    s["scales"] = np.full((P, 3), 0.01, np.float32)
    s["rotations"] = np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1))
    s["opacities"] = np.full((P, 1), OPACITY, np.float32)
    for k in ("means3D", "scales"):
        s[k][vis] = st[k]
    tile_of = np.full(P, -1, np.int64)
    tile_of[vis] = st["tile_of"]
    s.update(tile_of=tile_of, lengths_by_tile=st["lengths_by_tile"], z=s["means3D"][:, 2].copy(), gx=2, gy=2)
    return s


TOTALS = {f"total_{n}": (lambda n=n: total_scene(n, 60 + i)) for i, n in
          enumerate([2047, 2048, 2049, 8191, 8192, 8193, 16385])}
TOTALS.update({f"culled_{n}": (lambda n=n: total_scene(n, 70 + i, cull_third=True)) for i, n in
               enumerate([1, 2, 1023, 1024, 1025, 2049])})

GIANT_IDS = [0, 57, 58, 199]


def _giant():
    """200 ordinary splats on a 1024x768 image (64x48 tiles) and four huge ones (sigma 130 to 180 px: radius 400 px
    or more, a rectangle at least 50 tiles wide over all 48 rows), two of them with consecutive ids"""
    s = make_scene(200, 1024, 768, seed=7, sh_degree=0, log_scale=math.log(0.05))
    rng = np.random.default_rng(77)
    for k, i in enumerate(GIANT_IDS):
        s["means3D"][i] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 4.0 + 0.25 * k]
        s["scales"][i] = [0.8, 0.6 + 0.05 * k, 0.7]
        s["opacities"][i] = 0.2 + 0.2 * k
    return s


def _indef_small():
    import rule_scenes as RS
    return RS.scene("indef_small")


def _plain(**kw):
    return lambda: dict(s=make_scene(**kw), cov3D=None)


AUDITS = {
    "sh3000": _plain(P=3000, W=160, H=96, seed=0),
    "sh5000": _plain(P=5000, W=257, H=129, seed=2, sh_degree=2),
    "big800": _plain(P=800, W=160, H=96, seed=12, log_scale=math.log(0.2)),
    "sh4000": _plain(P=4000, W=200, H=120, seed=3, sh_degree=1),
    "giant": lambda: dict(s=_giant(), cov3D=None),
    "indef_small": _indef_small,
}
GENERAL_AUDITS = ["sh3000", "sh5000", "big800", "sh4000", "giant"]  # >= 500 pairs of each kind

_SCENES, _ORACLE, _REACH = {}, {}, {}


def scene(name):
    """dict(s = the scene, cov3D = its cov3D_precomp or None)"""
    if name not in _SCENES:
        if name in AUDITS:
            sc = AUDITS[name]()
            _SCENES[name] = dict(s=sc["s"], cov3D=sc["cov3D"])
        else:
            _SCENES[name] = dict(s=(STACKS.get(name) or TOTALS[name])(), cov3D=None)
    return _SCENES[name]


def oracle_run(O, name):
    """The oracle's forward of the scene, made once: dict(nr, color, depth, radii, state, export); an all-culled
    scene has no state and an export of empty lists."""
    if name not in _ORACLE:
        from gpu_helpers import o_forward
        sc = scene(name)
        s = sc["s"]
        nr, color, depth, radii, st = o_forward(O, s, cov3D=sc["cov3D"])
        T = ((s["W"] + 15) // 16) * ((s["H"] + 15) // 16)
        ex = st.export() if st is not None and st.handle else None
        if ex is None or nr == 0:
            ex = dict(point_list=np.zeros(0, np.uint32), ranges=np.zeros((T, 2), np.uint32), L=0,
                      depths=s["means3D"][:, 2].copy(), tiles_touched=np.zeros(len(radii), np.uint32))
        _ORACLE[name] = dict(nr=nr, color=color, depth=depth, radii=radii, state=st, export=ex)
    return _ORACLE[name]


def gpu_lists(C, name):
    """One HIP forward of the scene on cuda:0 and its lists: (fwd = rasterize_gaussians' tuple, lists = dict of numpy
    arrays ranges (T, 2), order, n = L', gid, reach, slot, depth from debug_tile_lists)"""
    import torch
    from gpu_helpers import c_forward, to_dev
    sc = scene(name)
    s = sc["s"]
    dev = torch.device("cuda:0")
    cov = None if sc["cov3D"] is None else torch.tensor(sc["cov3D"], device=dev)
    fwd = c_forward(C, s, to_dev(s, dev), cov3D=cov)
    out = C.debug_tile_lists(fwd[4], fwd[5], fwd[6], len(s["means3D"]), int(s["W"]), int(s["H"]), fwd[0])
    keys = ("ranges", "order", "n", "gid", "reach", "slot", "depth")
    lists = {k: (v if k == "n" else v.cpu().numpy()) for k, v in zip(keys, out)}
    return fwd, lists


def digests(fwd, lists):
    """(SHA-256 over ranges, gid and reach; SHA-256 over the colour and depth images)"""
    import hashlib
    h = hashlib.sha256()
    for k in ("ranges", "gid", "reach"):
        h.update(np.ascontiguousarray(lists[k]).tobytes())
    g = hashlib.sha256()
    for t in fwd[1:3]:
        g.update(t.cpu().numpy().tobytes())
    return h.hexdigest(), g.hexdigest()


# ---- list algebra (numpy, exact) ---------------------------------------------------------------------------------
def tiles_of_positions(ranges, n):
    """tile of each list position 0 .. n - 1 from (T, 2) ranges that partition [0, n) in tile order (which
    structure_errors checks first)"""
    r = np.asarray(ranges, np.int64)
    out = np.repeat(np.arange(len(r), dtype=np.int64), r[:, 1] - r[:, 0])
    assert len(out) == n
    return out


def depth_bits(z):
    return np.ascontiguousarray(np.asarray(z, np.float32)).view(np.uint32)


def lexsort_lists(tile_of, z, T):
    """(ranges (T, 2), gid list): every Gaussian with tile_of >= 0 in its tile, by (depth bits, id) -- numpy's
    lexsort, the reference's within-tile order"""
    ids = np.nonzero(np.asarray(tile_of) >= 0)[0]
    o = np.lexsort((ids, depth_bits(z)[ids], np.asarray(tile_of)[ids]))
    gid = ids[o]
    counts = np.bincount(np.asarray(tile_of)[ids], minlength=T)
    ends = np.cumsum(counts)
    ranges = np.stack([ends - counts, ends], 1)
    ranges[counts == 0] = 0
    return ranges, gid


def structure_errors(lists, T, num_rendered, P):
    """Violations of the lists' structure (empty = none).  lists: dict(ranges (T, 2), order (T,), n, gid, reach,
    slot, depth) as numpy arrays, gs4d_debug_tile_lists' outputs."""
    err = []
    r = np.asarray(lists["ranges"], np.int64)
    n = int(lists["n"])
    if not (0 <= n <= num_rendered):
        err.append(f"L' = {n} outside [0, num_rendered = {num_rendered}]")
    if r.shape != (T, 2) or any(len(lists[k]) != n for k in ("gid", "reach", "slot", "depth")):
        return err + ["shapes"]
    ne = r[:, 1] > r[:, 0]
    if np.any(r[~ne] != 0):
        err.append("an empty tile's range is not (0, 0)")
    st, en = r[ne, 0], r[ne, 1]
    if ne.any():
        if st[0] != 0 or en[-1] != n or np.any(st[1:] != en[:-1]):
            err.append("the ranges do not partition [0, L') in tile order")
    elif n != 0:
        err.append("no ranges but L' > 0")
    order = np.asarray(lists["order"], np.int64)
    if not np.array_equal(np.sort(order), np.arange(T)):
        err.append("order is not a permutation of the tiles")
    else:
        key = np.minimum(r[order, 1] - r[order, 0], 1023)
        if np.any(np.diff(key) > 0):
            err.append("order: min(len, 1023) increases somewhere")
    gid = np.asarray(lists["gid"], np.int64)
    if n and (gid.min() < 0 or gid.max() >= P):
        err.append("a gid out of range")
    if n and (np.asarray(lists["slot"], np.int64).min() < 0 or np.asarray(lists["slot"], np.int64).max() >= num_rendered
              or len(np.unique(lists["slot"])) != n):
        err.append("the slots are not distinct values below num_rendered")
    if not err and n:
        tile = tiles_of_positions(r, n)
        if len(np.unique(tile * P + gid)) != n:
            err.append("a (tile, gid) pair appears twice")
    return err


def order_errors(lists, want_depth):
    """Violations of the order inside the tiles: keys (bits of the returned depth, gid) strictly increasing, slot
    increasing wherever gid is (the emission-slot tie-break claim), returned depths = want_depth[gid] bitwise."""
    err = []
    n = int(lists["n"])
    if n == 0:
        return err
    gid = np.asarray(lists["gid"], np.int64)
    tile = tiles_of_positions(lists["ranges"], n)
    bits = depth_bits(lists["depth"]).astype(np.uint64)
    key = (bits << np.uint64(32)) | gid.astype(np.uint64)
    same = tile[1:] == tile[:-1]
    bad = same & ~(key[1:] > key[:-1])
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        lens = np.bincount(tile)
        err.append(f"{int(bad.sum())} adjacent pairs out of (depth bits, gid) order, first at list position {i + 1} "
                   f"(tile {tile[i]}), in tiles of length {sorted(set(lens[tile[1:][bad]].tolist()))}")
    if not np.array_equal(bits, depth_bits(want_depth)[gid].astype(np.uint64)):
        err.append("a returned depth differs from the Gaussian's view depth")
    o = np.lexsort((gid, tile))
    slot = np.asarray(lists["slot"], np.int64)[o]
    if np.any((tile[o][1:] == tile[o][:-1]) & ~(slot[1:] > slot[:-1])):
        err.append("inside a tile the emission slot does not increase with the Gaussian id")
    return err


def pair_keys(ranges, gid, P):
    return tiles_of_positions(ranges, len(gid)) * np.int64(P) + np.asarray(gid, np.int64)


def oracle_order_errors(lists, ex, P):
    """The gid sequence of each tile must equal the oracle's point_list restricted to the emitted pairs (which also
    makes the emitted pairs a subset of the oracle's)."""
    mine = pair_keys(lists["ranges"], lists["gid"], P)
    ref = pair_keys(ex["ranges"], ex["point_list"], P)
    kept = ref[np.isin(ref, mine)]
    if len(kept) != len(mine):
        return [f"{len(mine) - len(kept)} emitted pairs are not in the oracle's list"]
    if not np.array_equal(kept, mine):
        return [f"{int((kept != mine).sum())} list positions differ from the oracle's order"]
    return []


# ---- the fp64 alpha test ------------------------------------------------------------------------------------------
def reach_reference(s, ex):
    """For every (tile, Gaussian) pair of the oracle's list and each 8-row half tile, in float64 from the oracle's
    conic_opacity and means2D: the maximum over the pixel centres inside the image of min(0.99, o exp(power))
    (forward.cu:330-348; a pixel with power > 0 counts as 0).  A (pair, half) is reachable when that is >= 1/255.
    Returns dict(key (N,) = tile P + gid, tile, gid, amax (N, 2), need (N,) bits of the reachable halves, exists (N,)
    bits of the halves with a row inside the image, nonpd (N,): the conic is not positive definite in fp32, the
    culling's own test)."""
    P, W, H = len(ex["conic_opacity"]), s["W"], s["H"]
    gx = (W + 15) // 16
    gid = np.asarray(ex["point_list"], np.int64)
    tile = tiles_of_positions(ex["ranges"], len(gid))
    co = np.asarray(ex["conic_opacity"], np.float64)[gid]
    m = np.asarray(ex["means2D"], np.float64)[gid]
    amax = np.zeros((len(gid), 2))
    exists = np.zeros(len(gid), np.uint8)
    lx, ly = np.meshgrid(np.arange(16), np.arange(8))
    for h in (0, 1):
        for c0 in range(0, len(gid), 1 << 15):
            sl = slice(c0, c0 + (1 << 15))
            px = (16 * (tile[sl] % gx))[:, None] + lx.reshape(-1)[None, :]
            py = (16 * (tile[sl] // gx) + 8 * h)[:, None] + ly.reshape(-1)[None, :]
            inside = (px < W) & (py < H)
            dx, dy = m[sl, 0:1] - px, m[sl, 1:2] - py
            power = -0.5 * (co[sl, 0:1] * dx * dx + co[sl, 2:3] * dy * dy) - co[sl, 1:2] * dx * dy
            with np.errstate(over="ignore"):
                alpha = np.minimum(0.99, co[sl, 3:4] * np.exp(np.minimum(power, 0.0)))
            alpha = np.where(inside & (power <= 0), alpha, 0.0)
            amax[sl, h] = alpha.max(1)
            exists[sl] |= (inside.any(1).astype(np.uint8) << h)
    need = ((amax[:, 0] >= ALPHA_MIN).astype(np.uint8) | ((amax[:, 1] >= ALPHA_MIN).astype(np.uint8) << 1))
    c32 = np.asarray(ex["conic_opacity"], np.float32)[gid]
    a, b, c = c32[:, 0], c32[:, 1], c32[:, 2]
    nonpd = ~((a > 0) & (c > 0) & (a * c - b * b > 0))
    return dict(key=tile * np.int64(P) + gid, tile=tile, gid=gid, amax=amax, need=need, exists=exists, nonpd=nonpd)


def reach_of(O, name):
    if name not in _REACH:
        _REACH[name] = reach_reference(scene(name)["s"], oracle_run(O, name)["export"])
    return _REACH[name]


def reach_stats(ref):
    need = ref["need"]
    rel = np.abs(ref["amax"] * 255.0 - 1.0)
    return dict(pairs=len(need), reachable=int((need != 0).sum()), unreachable=int((need == 0).sum()),
                one_half=int(((need == 1) | (need == 2)).sum()), nonpd=int(ref["nonpd"].sum()),
                near=int((rel < 1e-4).any(1).sum()))


def culling_errors(lists, ref, P):
    """Every reachable (pair, half) must be emitted with its bit set; a pair whose conic is not positive definite
    must be there with every existing half's bit.  Returns (errors, share of the emitted pairs no half of which is
    reachable: the cost of the continuous-rectangle bound)."""
    mine = pair_keys(lists["ranges"], lists["gid"], P)
    o = np.argsort(mine, kind="stable")
    ms, mr = mine[o], np.asarray(lists["reach"], np.uint8)[o]
    pos = np.searchsorted(ms, ref["key"])
    found = (pos < len(ms)) & (ms[np.minimum(pos, max(len(ms) - 1, 0))] == ref["key"]) if len(ms) else \
        np.zeros(len(ref["key"]), bool)
    got = np.where(found, mr[np.minimum(pos, max(len(ms) - 1, 0))] if len(ms) else 0, 0).astype(np.uint8)
    err = []
    if np.any(got & ~ref["exists"]):
        err.append("a reach bit is set for a half tile outside the image")
    miss = ref["need"] & ~got
    if miss.any():
        i = int(np.nonzero(miss)[0][0])
        err.append(f"{int((miss != 0).sum())} pairs lack a reachable half: e.g. tile {ref['tile'][i]} gid "
                   f"{ref['gid'][i]} need {ref['need'][i]} got {got[i]} max alpha x 255 = {ref['amax'][i] * 255}")
    npd = ref["nonpd"]
    if np.any(got[npd] != ref["exists"][npd]):
        err.append(f"{int((got[npd] != ref['exists'][npd]).sum())} pairs with a conic that is not positive definite "
                   "are culled or lack an existing half")
    if int(found.sum()) != len(mine):
        err.append(f"{len(mine) - int(found.sum())} emitted pairs are not in the oracle's list")
    wasted = float(((got != 0) & (ref["need"] == 0)).sum()) / max(len(mine), 1)
    return err, wasted
