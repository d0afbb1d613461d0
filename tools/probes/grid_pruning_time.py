"""Grid-pruning timing (GPU): gs4d_train._C.voxel_downsample on clustered clouds of 100k, 1M and 4M points at the
voxel size grid_pruning picks without cameras (bounding box diagonal / 100), against the host numpy formulation
of the same thing (tests/voxel_refs.py) in the same process.

The device figure is HIP events around 20 back-to-back calls (each call synchronises twice and copies its M rows
out, so this is the time a caller sees), median [min, max] of 7 rounds; the host figure is wall clock, median of 3.
The reference's own path (Open3D's voxel_down_sample) is not installed on the project's machines and is not timed.

    python tools/probes/grid_pruning_time.py [--sizes 100000,1000000,4000000] [--no-host] [--rounds 7] [--calls 20]

The per-kernel figures of DESIGN 10.6 are a kernel trace of one size at a time, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o voxel -- \
        python tools/probes/grid_pruning_time.py --sizes 1000000 --no-host --rounds 2 --calls 10
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxel_refs  # noqa: E402
from gs4d_train import _C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="100000,1000000,4000000")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
assert torch.cuda.is_available(), "this probe measures the GPU"

for n in (int(s) for s in args.sizes.split(",")):
    pts, cols = voxel_refs.clustered_cloud(n, seed=0)
    voxel = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)) / 100.0)
    p, c = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()
    for _ in range(3):
        out = _C.voxel_downsample(p, c, voxel)
    m = out[0].shape[0]
    rounds = []
    for _ in range(args.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            _C.voxel_downsample(p, c, voxel)
        t1.record()
        torch.cuda.synchronize()
        rounds.append(t0.elapsed_time(t1) / args.calls * 1e3)
    line = (f"N={n} voxel={voxel:.5f} M={m} (M/N={m / n:.4f}): device {statistics.median(rounds):.1f} us "
            f"[{min(rounds):.1f}, {max(rounds):.1f}] per call")
    if not args.no_host:
        host = []
        for _ in range(3):
            t = time.perf_counter()
            keys, counts, hp, hc = voxel_refs.voxel_downsample(pts, cols, voxel)
            host.append((time.perf_counter() - t) * 1e3)
        same = len(keys) == m and int(voxel_refs.ulp_distance(out[0].cpu().numpy(), hp).max()) <= 1
        line += f"; host numpy {statistics.median(host):.1f} ms [{min(host):.1f}, {max(host):.1f}]; agree: {same}"
    print(line, flush=True)
