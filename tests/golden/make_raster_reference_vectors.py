"""Record runs of the reference's OWN rasterizer and simple-knn (build container only).

oracle/ref_cpu/build_ref.py compiles the reference's cuda_rasterizer and simple-knn sources for the host against a
CUDA-on-CPU shim (oracle/_ref/libgs4d_ref.so; nothing of it is committed).  This script runs that build on every
fixture scene of tests/reference_scenes.py and writes what it computed:

  tests/golden/ref_raster_<name>.npz   in_*          the scene: every input of the entry points (reference_scenes.inputs_of);
                                                     for DIGEST_ONLY scenes, whose file would pass MAX_BYTES with them
                                                     (term2: 180 KB), in_digest, the inputs' SHA-256: the scene is then
                                                     tests/rule_scenes.py's by name, verified against the digest
                                       g             the upstream colour gradient (+-1, from the reference's own image)
                                       color, depth, radii, num_rendered
                                       dL_dmeans2D ... dL_drotations (parity.GRAD_NAMES), dL_dconic
                                       st_*          the exported state (reference_scenes.STATE_KEYS), read through the
                                                     reference's own GeometryState / BinningState / ImageState fromChunk
  tests/golden/ref_knn_vectors.npz     <cloud>_x, <cloud>_d: the clouds of tests/test_knn.py cut to KNN_MAX_POINTS points
                                       and five tiny ones (1, 2, 3, 4, 7 points), with SimpleKNN::knn's results

The run is single-threaded and deterministic, so running this again gives the same bytes in every array
(tests/test_reference_run.py::test_fixtures_are_the_reference_run checks it where the build is available).  No file may
exceed MAX_BYTES, the size of the largest fixture that was here before these (ref_sh_vectors.npz).

Usage (from the repository root, where the reference checkout exists):
    python tests/golden/make_raster_reference_vectors.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
for _p in (ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_BYTES = 142968
KNN_MAX_POINTS = 1500
KNN_TINY = (1, 2, 3, 4, 7)


DIGEST_ONLY = ("term2",)


def record(name):
    """the arrays of ref_raster_<name>.npz, from a run of the reference build"""
    import reference_scenes as S
    from oracle import ref as R
    sc = S.scene(name)
    r = S.run(R, sc)
    out = S.inputs_of(sc)
    if name in DIGEST_ONLY:
        out = dict(in_digest=S.digest_of(out))
    out.update(S.as_record(r))
    return out


def knn_clouds():
    """(name, points) of ref_knn_vectors.npz"""
    from test_knn import clouds
    for name, x in clouds():
        yield name, np.ascontiguousarray(x[:KNN_MAX_POINTS])
    rng = np.random.default_rng(11)
    for P in KNN_TINY:
        yield f"tiny{P}", rng.normal(size=(P, 3)).astype(np.float32)


def record_knn():
    from oracle import ref as R
    out = {}
    for name, x in knn_clouds():
        out[f"{name}_x"] = x
        out[f"{name}_d"] = R.knn_mean_dist(x)
    return out


def main():
    import reference_scenes as S
    from oracle import ref as R
    if not R.available():
        sys.exit("the reference checkout is not here: nothing to run")
    files = {f"ref_raster_{name}.npz": record(name) for name in S.FIXTURES}
    files["ref_knn_vectors.npz"] = record_knn()
    for fn, arrays in files.items():
        path = os.path.join(OUT, fn)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"{fn}: {size} bytes")
        if size > MAX_BYTES:
            sys.exit(f"{fn} is larger than {MAX_BYTES} bytes: shrink the scene")


if __name__ == "__main__":
    main()
