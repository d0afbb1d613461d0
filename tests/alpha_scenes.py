"""Two more scenes for the alpha-image tests (test infrastructure), next to those of tests/depth_scenes.py.

  opaque  P=200, 70x45, large splats of opacity 0.95: pixels whose walk terminates (final_T < 2e-4) next to pixels
          that stay mostly empty (final_T > 0.5); the 0.99 cap and the 1/255 rule bite here, so this scene is
          compared with the GPU's own results (identities), never with the fp64 restatement
  sparse  P=12, 70x45, small splats in the image's middle: most tiles have an empty list, most pixels no
          contributor
  behind  sparse with every Gaussian behind the camera: P > 0 and not one instance

tests/test_alpha_boundary.py asserts these properties through the CPU oracle.
"""
import math

import numpy as np

from gs4d_train.synthetic import make_scene

NAMES = ["opaque", "sparse", "behind"]
_CACHE = {}


def _opaque():
    s = make_scene(200, 70, 45, seed=11, sh_degree=3, log_scale=math.log(0.15), z_range=(2.0, 6.0))
    s["opacities"] = np.full_like(s["opacities"], 0.95)
    return s


def _sparse():
    return make_scene(12, 70, 45, seed=3, sh_degree=3, log_scale=math.log(0.03), z_range=(4.0, 6.0), spread=0.2)


def _behind():
    s = _sparse()
    s["means3D"] = (s["means3D"] * np.array([1, 1, -1], np.float32)).astype(np.float32)  # view z < 0 (identity camera)
    return s


def scene(name):
    """depth_scenes.scene's dict for one of NAMES (SH colours, scales and rotations)"""
    if name not in _CACHE:
        s = {"opaque": _opaque, "sparse": _sparse, "behind": _behind}[name]()
        _CACHE[name] = dict(name=name, s=s, colors=None, cov3D=None, use_sh=True, mode="sh")
    return _CACHE[name]


_REF = {}


def reference(O, name):
    """the oracle's forward of the scene, made once: dict(nr, color, depth, radii, final_T (H, W), n_contrib (H, W),
    ranges (tiles, 2))"""
    if name not in _REF:
        from gpu_helpers import o_forward
        s = scene(name)["s"]
        nr, color, depth, radii, st = o_forward(O, s)
        ex = st.export()
        _REF[name] = dict(nr=nr, color=color, depth=depth, radii=radii, final_T=np.asarray(ex["final_T"]),
                          n_contrib=np.asarray(ex["n_contrib"]), ranges=np.asarray(ex["ranges"]))
    return _REF[name]


def tile_is_empty(ref, H, W):
    """(H, W) bool: the pixel's 16x16 tile has an empty list"""
    gx = (W + 15) // 16
    lens = (ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]).reshape(-1)
    ys, xs = np.mgrid[0:H, 0:W]
    return lens[(ys // 16) * gx + xs // 16] == 0
