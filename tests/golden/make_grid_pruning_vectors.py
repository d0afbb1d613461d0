"""Regenerates tests/golden/grid_pruning_sizes.npz: the voxel sizes the REFERENCE's own utils/grid_pruning.py
computes for a handful of seeded clouds and camera lists.

    python tests/golden/make_grid_pruning_vectors.py /path/to/the/reference/checkout

The reference module is loaded from its file with a stand-in `open3d` in sys.modules (Open3D is not a dependency of
this repository): the stand-in's voxel_down_sample records the voxel size it is given and returns its input, so the
reference's compute_adaptive_voxel_size and grid_pruning run unchanged up to that call.  Only data is stored: each
case's seeds and parameters (JSON) and the recorded fp64 voxel size.  No test reads the reference checkout; the
tests rebuild the inputs from the seeds (tests/voxel_refs.py) and compare gs4d_train.pruning bitwise."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voxel_refs  # noqa: E402

# (kind, cloud seed, points, cloud scale, camera seed, cameras, extra arguments)
CASES = [
    ("adaptive", 1, 500, 1.0, 11, 0, {}),
    ("adaptive", 2, 500, 1.0, 12, 1, {}),
    ("adaptive", 3, 800, 2.0, 13, 3, {}),
    ("adaptive", 4, 1000, 1.5, 14, 12, {"scale_factor": 4.0}),
    ("adaptive", 5, 500, 1.0, 15, 3, {"focal_mean": 700.0}),
    ("adaptive", 6, 500, 1.0, 16, 3, {"depth_mean": 2.5}),
    ("adaptive", 7, 500, 1.0, 17, 0, {"focal_mean": 850.0, "depth_mean": 3.25, "scale_factor": 3.5}),
    ("adaptive", 8, 500, 1.0, 18, 1, {"focal_mean": 1.0e6}),        # the lower clamp: 0.001
    ("adaptive", 9, 500, 5000.0, 19, 0, {}),                         # the upper clamp: 1.0
    ("grid", 10, 600, 1.0, 20, 0, {}),                               # an empty camera list is still "adaptive"
    ("grid", 11, 600, 1.0, 21, 1, {}),
    ("grid", 12, 900, 2.0, 22, 3, {"static_scale": 5.0, "dynamic_scale": 2.0}),
    ("grid", 13, 900, 1.0, 23, 12, {}),
    ("grid", 14, 600, 3.0, 24, None, {}),                            # no cameras: bounding box diagonal / 100
    ("grid", 15, 600, 0.7, 25, 3, {"use_adaptive": False}),
]


def load_reference(root, recorded):
    o3d = types.ModuleType("open3d")

    class PointCloud:
        def __init__(self):
            self.points = self.colors = None

        def voxel_down_sample(self, voxel_size):
            recorded.append(voxel_size)
            return self

    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=np.asarray)
    sys.modules["open3d"] = o3d
    sys.path.insert(0, root)  # the module's own `from utils.graphics_utils import BasicPointCloud`
    spec = importlib.util.spec_from_file_location("reference_grid_pruning", os.path.join(root, "utils", "grid_pruning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    recorded = []
    ref = load_reference(root, recorded)
    from utils.graphics_utils import BasicPointCloud
    sizes = []
    for kind, seed, n, scale, cam_seed, k, extra in CASES:
        pts, cols = voxel_refs.golden_cloud(seed, n, scale)
        cams = None if k is None else voxel_refs.golden_cameras(cam_seed, k)
        if kind == "adaptive":
            sizes.append(ref.compute_adaptive_voxel_size(pts, cams, **extra))
        else:
            del recorded[:]
            ref.grid_pruning(BasicPointCloud(points=pts, colors=cols, normals=np.zeros((0, 3))), cameras=cams, **extra)
            assert len(recorded) == 1
            sizes.append(recorded[0])
    np.savez(os.path.join(HERE, "grid_pruning_sizes.npz"), cases=np.array(json.dumps(CASES)),
             voxel_size=np.array(sizes, dtype=np.float64))
    for case, s in zip(CASES, sizes):
        print(case, repr(float(s)))


if __name__ == "__main__":
    main(sys.argv[1])
