"""Host restatement of gs4d_voxel_downsample's semantics (include/gs4d.h) in fp64 numpy: the reference the
grid-pruning tests and tools/probes/grid_pruning_time.py compare against.  Not a test."""
import numpy as np


def _keys(points, voxel_size):
    """(the points as fp64, their linear voxel keys (N) int64)."""
    p = np.ascontiguousarray(points, dtype=np.float32).astype(np.float64)
    vs = float(voxel_size)
    origin = p.min(axis=0) - vs / 2
    idx = np.floor((p - origin) / vs).astype(np.int64)
    n = idx.max(axis=0) + 1
    return p, (idx[:, 2] * n[1] + idx[:, 1]) * n[0] + idx[:, 0]


def voxel_downsample(points, colors, voxel_size):
    """(keys (M) int64, counts (M) int64, points (M, 3) float32, colors (M, 3) float32 or None).

    origin = min - voxel_size / 2; index = floor((p - origin) / voxel_size) in fp64; key = (iz ny + iy) nx + ix
    with n* = largest index + 1; a stable argsort on the key; per-voxel fp64 sums by np.add.reduceat in sorted
    order, divided by the counts and rounded once to fp32."""
    p, key = _keys(points, voxel_size)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    counts = np.diff(np.r_[heads, ks.size])
    out_p = (np.add.reduceat(p[order], heads, axis=0) / counts[:, None]).astype(np.float32)
    out_c = None
    if colors is not None:
        c = np.ascontiguousarray(colors, dtype=np.float32).astype(np.float64)
        out_c = (np.add.reduceat(c[order], heads, axis=0) / counts[:, None]).astype(np.float32)
    return ks[heads], counts, out_p, out_c


def sorted_keys(points, voxel_size):
    """The linear key of every point, in the stable sorted order (what a row's run of points is read from)."""
    return np.sort(_keys(points, voxel_size)[1], kind="stable")


def ulp_distance(a, b):
    """Elementwise distance of two float32 arrays in units in the last place (+0 and -0 coincide)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


class GoldenCamera:
    """The fields utils/grid_pruning.py:66-78 reads of a camera; `ours` names them as gs4d_train.camera.Camera does."""

    def __init__(self, R, T, fovx, fovy, width, height, ours=False):
        self.R, self.T = R, T
        if ours:
            self.FoVx, self.FoVy, self.image_width, self.image_height = fovx, fovy, width, height
        else:
            self.FovX, self.FovY, self.width, self.height = fovx, fovy, width, height


def golden_cloud(seed, n, scale):
    """The seeded fp64 cloud of a golden case (tests/golden/grid_pruning_sizes.npz)."""
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, scale, (n, 3)), rng.uniform(0, 1, (n, 3))


def golden_cameras(seed, k, ours=False):
    """k seeded cameras: a random rotation (QR of a normal matrix), a translation of a few units, fields of view
    between 0.5 and 1.2 rad, image sizes between 320 and 1352."""
    rng = np.random.default_rng(seed)
    cams = []
    for _ in range(k):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        T = rng.normal(0.0, 3.0, 3)
        fovx, fovy = rng.uniform(0.5, 1.2, 2)
        width, height = (int(v) for v in rng.integers(320, 1353, 2))
        cams.append(GoldenCamera(q, T, float(fovx), float(fovy), width, height, ours))
    return cams


def clustered_cloud(n, seed=0, clusters=24, sigma=0.04, extent=1.0):
    """n float32 points around `clusters` centres in [-extent, extent]^3 (Gaussian blobs of width sigma), with
    colours in [0, 1): the structure-from-motion-like cloud of the tests and the timing probe."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-extent, extent, (clusters, 3))
    pts = centres[rng.integers(0, clusters, n)] + rng.normal(0.0, sigma, (n, 3))
    return pts.astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)
