"""Cost of the K-NN graph and of the fused isometry term (diagnostic, GPU).

Reports, the rows alternated inside every round of this one process after a warm-up of each, HIP events around CALLS
calls, microseconds per call, median [min .. max] over ROUNDS rounds:
  per cloud (clustered: normal blobs of sigma 0.1 around P / 400 centres, test_gpu_large_scene's recipe; 100k and 1M
  points): distCUDA2, knn_graph at K = 8 and K = 16;
  at P = 100k, K = 8, xb = xa + 0.05 * noise: the fused value + both gradients (one isometry_loss_and_grad call), the
  torch formulation forward + backward (gather, norm, index_add_ backward), and the fused call on a graph with one
  node of in-degree ~3000 (3000 copies of one point appended: that node is one lane looping).
No time bar is set: the rows are reported.  --small: 4,000 and 20,000 points (a rehearsal, not a measurement)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "4dgaussians-fast-train_amd")]
from gs4d_train.rigidity import build_graph, isometry_loss_and_grad  # noqa: E402
from simple_knn._C import distCUDA2, knn_graph  # noqa: E402

CALLS, ROUNDS = 5, 9


def timed_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(rows):
    for fn in rows.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in rows}
    for _ in range(ROUNDS):
        for k, fn in rows.items():
            res[k].append(timed_us(fn, CALLS))
    for k, v in res.items():
        print(f"  {k:44s} {statistics.median(v):10.1f} us  [{min(v):10.1f} .. {max(v):10.1f}]", flush=True)
    return res


def clustered(P, seed):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(max(1, P // 400), 3)) * 4
    return (c[rng.integers(0, len(c), P)] + rng.normal(size=(P, 3)) * 0.1).astype(np.float32)


def torch_term(xa, xb, idx):
    j = idx.long()
    ra = ((xa[:, None, :] - xa[j]).pow(2).sum(-1) + 1e-12).sqrt()
    rb = ((xb[:, None, :] - xb[j]).pow(2).sum(-1) + 1e-12).sqrt()
    return (rb - ra).pow(2).sum() / idx.numel()


def main():
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "rigidity_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    sizes = (4_000, 20_000) if small else (100_000, 1_000_000)
    print(f"rigidity_time: {CALLS} calls x {ROUNDS} alternating rounds; median [min .. max]")
    for P in sizes:
        x = torch.tensor(clustered(P, 5), device=dev)
        print(f"clustered cloud, P = {P}")
        alternate({"distCUDA2": lambda: distCUDA2(x), "knn_graph K = 8": lambda: knn_graph(x, 8),
                   "knn_graph K = 16": lambda: knn_graph(x, 16)})
    P = sizes[0]
    xa = torch.tensor(clustered(P, 5), device=dev)
    xb = xa + 0.05 * torch.randn_like(xa)
    g = build_graph(xa, 8)
    hub = torch.cat([xa, xa[:1].expand(3000 if not small else 300, 3)])
    hub_b = hub + 0.05 * torch.randn_like(hub)
    gh = build_graph(hub, 8)
    deg = (gh.in_start[1:] - gh.in_start[:-1])
    print(f"isometry term, P = {P}, K = 8 (the hub graph: P = {hub.shape[0]}, max in-degree {int(deg.max())})")

    def torch_fwd_bwd():
        a, b = xa.detach().requires_grad_(True), xb.detach().requires_grad_(True)
        torch_term(a, b, g.idx).backward()
        return a.grad, b.grad
    alternate({"fused value + both gradients": lambda: isometry_loss_and_grad(xa, xb, g, 1.0),
               "torch formulation forward + backward": torch_fwd_bwd,
               "fused, one node of in-degree ~3000": lambda: isometry_loss_and_grad(hub, hub_b, gh, 1.0)})


if __name__ == "__main__":
    main()
