"""The scenes on which the reference's own rasterizer (oracle/ref.py, built for the host) is run (test infrastructure).

FIXTURES  small scenes whose reference runs are recorded under tests/golden/ref_raster_<name>.npz
          (tests/golden/make_raster_reference_vectors.py) and compared with the oracle on the CPU and with the HIP
          kernels on the GPU.  On every one `oracle.flip_flags` with parity.FLIP_BAND_ALPHA / FLIP_BAND_T flags no pixel
          and no Gaussian (tests/test_reference_run.py asserts it), so a comparison against a fixture needs no flip
          allowance.  Seeds were passed over until that held; the condition was never relaxed.
LIVE      larger scenes that only the CPU test runs, next to the oracle, where the reference build is available.

The scenes that tests/rule_scenes.py names are reused under their names.  `scene(name)` returns rule_scenes.scene's
dict(s = make_scene's dict, colors / cov3D = precomputed inputs or None, use_sh); the SH degree and the modifier are
s["sh_degree"] and s["scale_modifier"], the coefficient rows s["shs"].shape[1].
"""
import math

import numpy as np

import rule_scenes as RS
from gs4d_train.synthetic import make_scene, make_upstream_grad

RULE_FIXTURES = ["clamp1", "clampmod7", "clamp_colors4", "indef_small_colors", "term2"]


def _rows(s, M, seed):
    """the scene with M coefficient rows: the first min(M, 16) kept, any beyond 16 drawn afresh"""
    P = s["shs"].shape[0]
    sh = np.zeros((P, M, 3), np.float32)
    k = min(M, 16)
    sh[:, :k] = s["shs"][:, :k]
    if M > 16:
        sh[:, 16:] = np.random.default_rng(seed + 500).normal(0, 0.1, (P, M - 16, 3))
    s["shs"] = sh
    return s


def _mid(P, W, H, seed, deg):
    """splats of a few pixels with mid opacities: several tiles each, lists of tens"""
    return make_scene(P, W, H, seed=seed, sh_degree=deg, log_scale=math.log(0.06), z_range=(2.0, 6.0))


def _sh3_m16(seed):
    return _mid(150, 48, 32, seed, 3)


def _sh1_m4(seed):
    return _rows(_mid(150, 50, 35, seed, 1), 4, seed)


def _sh0_m25(seed):
    return _rows(_mid(120, 50, 35, seed, 0), 25, seed)


def _depth_ties(seed):
    s = _mid(180, 64, 40, seed, 2)
    s["means3D"][:, 2] = np.round(s["means3D"][:, 2])  # five distinct depths: the binning's id tie order shows
    return s


def _bg_black(seed):
    s = _mid(150, 60, 33, seed, 3)
    s["bg"] = np.zeros(3, np.float32)
    return s


def _all_culled(seed):
    s = make_scene(40, 40, 24, seed=seed)
    s["means3D"][:, 2] = 0.1  # behind the 0.2 near plane: background everywhere, zero gradients
    return s


# seeds: the first on which no pixel and no Gaussian is flagged (see the module docstring); depth_ties_small seed 0
# has one flagged pixel and Gaussian
OWN_FIXTURES = [
    dict(name="sh3_m16", make=_sh3_m16, seed=0),
    dict(name="sh1_m4", make=_sh1_m4, seed=0),
    dict(name="sh0_m25", make=_sh0_m25, seed=0),
    dict(name="depth_ties_small", make=_depth_ties, seed=1),
    dict(name="bg_black", make=_bg_black, seed=0),
    dict(name="all_culled", make=_all_culled, seed=0),
]
FIXTURES = [e["name"] for e in OWN_FIXTURES[:3]] + RULE_FIXTURES + [e["name"] for e in OWN_FIXTURES[3:]]


def _deg(deg):
    return lambda: make_scene(1500, 129, 97, seed=40 + deg, sh_degree=deg)


def _big_splats_mod():
    s = make_scene(800, 160, 96, seed=12, log_scale=math.log(0.2))
    s["scale_modifier"] = 0.7
    return s


def _opaque_stack():
    s = make_scene(3000, 128, 128, seed=13, log_scale=math.log(0.1))
    s["opacities"] = np.full_like(s["opacities"], 0.995)
    return s


def _depth_ties_live():
    s = make_scene(3000, 160, 96, seed=20)
    s["means3D"][:, 2] = np.round(s["means3D"][:, 2] * 4) / 4
    return s


def _long_tiles():
    s = make_scene(5000, 64, 48, seed=19, log_scale=math.log(0.3))
    s["opacities"] = np.full_like(s["opacities"], 0.03)
    return s


def _huge_splat():
    """Gaussian 0 covers every one of the 16 x 10 = 160 tiles (more than 128)"""
    s = make_scene(400, 256, 160, seed=23)
    s["means3D"][0] = (0.0, 0.0, 5.0)
    s["scales"][0] = (2.5, 2.0, 1.5)
    s["opacities"][0] = 0.3
    return s


LIVE_MAKERS = dict(deg0=_deg(0), deg1=_deg(1), deg2=_deg(2), deg3=_deg(3), big_splats_mod=_big_splats_mod,
                   opaque_stack=_opaque_stack, depth_ties=_depth_ties_live, long_tiles=_long_tiles,
                   huge_splat=_huge_splat)
LIVE = list(LIVE_MAKERS)
_CACHE = {}


def scene(name):
    if name in _CACHE:
        return _CACHE[name]
    if name in RULE_FIXTURES:
        sc = RS.scene(name)
    else:
        own = {e["name"]: e for e in OWN_FIXTURES}
        s = own[name]["make"](own[name]["seed"]) if name in own else LIVE_MAKERS[name]()
        sc = dict(name=name, s=s, colors=None, cov3D=None, use_sh=True)
    _CACHE[name] = sc
    return sc


def upstream(color, s):
    """dL/dcolour (3, H, W) of an L1 loss against a uniform-random image, scaled to +-1 (make_upstream_grad x 3WH).
    `color` is the REFERENCE run's image, so that a fixture's upstream gradient does not depend on the oracle."""
    return (make_upstream_grad(np.asarray(color, np.float32))[0] * (3 * s["W"] * s["H"])).astype(np.float32)


INPUT_KEYS = ("bg", "means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix", "campos")


def inputs_of(sc):
    """the arrays and settings a fixture records: everything the rasterizer's entry points take"""
    s = sc["s"]
    out = {f"in_{k}": np.ascontiguousarray(np.asarray(s[k], np.float32)) for k in INPUT_KEYS}
    out["in_settings"] = np.array([s["tanfovx"], s["tanfovy"], s["scale_modifier"]], np.float64)
    out["in_dims"] = np.array([s["W"], s["H"], s["sh_degree"], int(sc["use_sh"])], np.int32)
    if sc["colors"] is not None:
        out["in_colors"] = np.asarray(sc["colors"], np.float32)
    if sc["cov3D"] is not None:
        out["in_cov3D"] = np.asarray(sc["cov3D"], np.float32)
    return out


def digest_of(inputs):
    """SHA-256 over inputs_of's arrays (names, shapes, types and bytes), as a uint8 array"""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(inputs):
        a = np.ascontiguousarray(inputs[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def scene_of(fx, name):
    """The scene dict of a loaded fixture (the inverse of inputs_of): nothing is regenerated.  The one fixture too
    large to hold its inputs within the size limit of tests/golden (term2; its SH table and the table's gradient are
    two thirds of the limit) records their SHA-256 instead: its scene is tests/rule_scenes.py's, by name, and must
    hash to the recorded digest."""
    if "in_digest" in fx:
        sc = scene(name)
        assert np.array_equal(digest_of(inputs_of(sc)), fx["in_digest"]), \
            f"{name}: the regenerated scene is not the one the reference run was recorded on"
        return sc
    s = {k: np.asarray(fx[f"in_{k}"]) for k in INPUT_KEYS}
    s["tanfovx"], s["tanfovy"], s["scale_modifier"] = (float(v) for v in fx["in_settings"])
    W, H, deg, use_sh = (int(v) for v in fx["in_dims"])
    s.update(W=W, H=H, sh_degree=deg)
    return dict(s=s, colors=np.asarray(fx["in_colors"]) if "in_colors" in fx else None,
                cov3D=np.asarray(fx["in_cov3D"]) if "in_cov3D" in fx else None, use_sh=bool(use_sh))


STATE_KEYS = ("depths", "means2D", "cov3D", "conic_opacity", "rgb", "clamped", "tiles_touched", "point_list", "ranges",
              "final_T", "n_contrib")


def replay_walk(rec, W, H):
    """The forward walk's DECISIONS per pixel, replayed in fp64 from a recorded run's state (st_means2D,
    st_conic_opacity, st_point_list, st_ranges): valid on the fixture scenes, where no decision lies near a threshold.
    Returns (last (H, W): the reference's n_contrib, the 1-based list position of the last blended splat;
    bound (H, W): the list position of the terminating splat, or the list's length for a pixel that never terminated,
    an upper bound of `last` with only skipped splats between; final_T (H, W); term_gid (H, W): the terminating
    Gaussian, -1 for a pixel that never terminated; blended: per tile, the set of Gaussians that blended into one of
    its pixels)."""
    xy = np.asarray(rec["st_means2D"], np.float64)
    con = np.asarray(rec["st_conic_opacity"], np.float64)
    plist, ranges = np.asarray(rec["st_point_list"]), np.asarray(rec["st_ranges"])
    last, bound = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    final_T = np.ones((H, W))
    term_gid, blended = np.full((H, W), -1, np.int64), []
    gx = (W + 15) // 16
    for tile, (a, b) in enumerate(ranges):
        y0, x0 = 16 * (tile // gx), 16 * (tile % gx)
        py, px = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        T = np.ones(py.shape)
        live = np.ones(py.shape, bool)
        lst, bnd = np.zeros(py.shape, np.int64), np.full(py.shape, int(b) - int(a), np.int64)
        tg, used = np.full(py.shape, -1, np.int64), set()
        for pos, g in enumerate(plist[int(a):int(b)]):
            dx, dy = xy[g, 0] - px, xy[g, 1] - py
            power = -0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) - con[g, 1] * dx * dy
            alpha = np.minimum(0.99, con[g, 3] * np.exp(np.minimum(power, 0.0)))
            blend = live & (power <= 0) & (alpha >= 1.0 / 255.0)
            test_T = T * (1 - alpha)
            ends = blend & (test_T < 1e-4)
            bnd[ends], tg[ends], live[ends] = pos, int(g), False
            blend &= ~ends
            T[blend] = test_T[blend]
            lst[blend] = pos + 1
            if blend.any():
                used.add(int(g))
        last[py, px], bound[py, px], final_T[py, px], term_gid[py, px] = lst, bnd, T, tg
        blended.append(used)
    return last, bound, final_T, term_gid, blended


def as_record(r):
    """a run's results under the names a fixture records them by (tests/golden/make_raster_reference_vectors.py)"""
    from oracle.parity import GRAD_NAMES
    out = dict(g=r["g"], color=r["color"], depth=r["depth"], radii=r["radii"], num_rendered=np.array(r["nr"], np.int32),
               dL_dconic=r["dconic"])
    out.update(dict(zip(GRAD_NAMES, r["grads"])))
    out.update({f"st_{k}": r["export"][k] for k in STATE_KEYS})
    return out


def run(E, sc, g=None):
    """Forward, backward and state export of the scene by engine E (oracle.oracle or oracle.ref: same call shapes).
    g: the upstream colour gradient; None derives it from this run's own image (`upstream`).  Returns dict(nr, color,
    depth, radii, g, grads = the 8-tuple, dconic, export, state)."""
    from gpu_helpers import o_forward
    s, colors, cov3D = sc["s"], sc["colors"], sc["cov3D"]
    nr, color, depth, radii, st = o_forward(E, s, colors=colors, cov3D=cov3D, use_sh=sc["use_sh"])
    if g is None:
        g = upstream(color, s)
    grads, dconic = E.rasterize_backward(
        st, s["bg"], s["means3D"], radii, colors, None if cov3D is not None else s["scales"],
        None if cov3D is not None else s["rotations"], s["scale_modifier"], cov3D, s["viewmatrix"], s["projmatrix"],
        s["tanfovx"], s["tanfovy"], g, s["shs"] if sc["use_sh"] else None, s["sh_degree"], s["campos"])
    return dict(nr=nr, color=color, depth=depth, radii=radii, g=g, grads=grads, dconic=dconic, export=st.export(),
                state=st)
