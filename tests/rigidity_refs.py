"""References and clouds of the K-NN graph and the local-isometry term (tests/test_rigidity_boundary.py,
tests/test_rigidity_gpu.py).

K-NN: a numpy brute force, fp32 distances as (dx*dx + dy*dy) + dz*dz (gs4d_knn_graph's own arithmetic, so the
distances agree bit for bit), self set to inf, rows ordered by (distance, index); the transpose is a stable argsort of
the valid edge ids by target.  Loss: the formula in torch -- fp64 autograd is the reference, its fp32 twin measures
the error an unfused fp32 formulation makes on the same inputs (the yardstick e_u of the bar max(4 e_u, 1e-6)).
"""
import functools

import numpy as np
import torch

FLT_MAX = np.float32(3.4028234663852886e38)
EPS = 1e-12


# ---- clouds ---------------------------------------------------------------------------------------------------------
def _gauss():
    return np.random.default_rng(7).normal(size=(3000, 3)).astype(np.float32)


def _lattice():
    g = np.arange(12, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).copy()


def _hub():
    d = np.random.default_rng(7).normal(size=(1500, 3)).astype(np.float32)
    return np.concatenate([d, np.repeat(d[:1], 300, 0), np.full((1, 3), 50.0, np.float32)])


def _knn_test_clouds():
    """test_knn.py's far_from_origin, clustered and plane_z0, drawn as there (one generator, in its order)"""
    rng = np.random.default_rng(7)
    rng.normal(size=(3000, 3))
    far = (rng.uniform(-1, 1, (2500, 3)) + np.array([50.0, -80.0, 120.0])).astype(np.float32)
    c = rng.normal(size=(40, 3)) * 10
    clustered = (c[rng.integers(0, 40, 4000)] + rng.normal(size=(4000, 3)) * 0.05).astype(np.float32)
    plane = rng.uniform(-2, 2, (2000, 3)).astype(np.float32)
    plane[:, 2] = 0.0
    return far, clustered, plane


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name in ("far_from_origin", "clustered", "plane_z0"):
        x = dict(zip(("far_from_origin", "clustered", "plane_z0"), _knn_test_clouds()))[name]
    else:
        x = {"gauss": _gauss, "lattice": _lattice, "hub": _hub}[name]()
    x.setflags(write=False)
    return x


CLOUDS = ("gauss", "lattice", "hub", "far_from_origin", "clustered", "plane_z0")
LOSS_CLOUDS = ("gauss", "lattice", "hub")


def large_clustered():
    """test_knn.py's test_gpu_large_scene cloud: 200,000 points around 500 centres"""
    rng = np.random.default_rng(5)
    c = rng.normal(size=(500, 3)) * 4
    return (c[rng.integers(0, 500, 200_000)] + rng.normal(size=(200_000, 3)) * 0.1).astype(np.float32)


# ---- K-NN -----------------------------------------------------------------------------------------------------------
def dist2_rows(x, rows):
    """fp32 squared distances from the points `rows` to every point, (dx*dx + dy*dy) + dz*dz, self = inf"""
    x = np.asarray(x, np.float32)
    d = x[None, :, :] - x[rows, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[np.arange(len(rows)), rows] = np.inf
    return d2


def knn_rows(x, K, rows):
    """(idx, dist2) of the given rows: ascending by (distance, index), -1 / FLT_MAX beyond min(K, P - 1)"""
    P = x.shape[0]
    rows = np.asarray(rows)
    idx = np.full((len(rows), K), -1, np.int32)
    dist = np.full((len(rows), K), FLT_MAX, np.float32)
    kv = min(K, P - 1)
    chunk = max(1, min(512, (1 << 23) // max(P, 1)))  # rows per block of the distance matrix
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        d2 = dist2_rows(x, r)
        for q in range(len(r)):
            if kv == 0:
                continue
            # only the points no farther than the kv-th smallest distance can enter: lexsort those
            cand = np.nonzero(d2[q] <= np.partition(d2[q], kv - 1)[kv - 1])[0]
            order = cand[np.lexsort((cand, d2[q][cand]))][:kv]
            idx[a + q, :kv] = order
            dist[a + q, :kv] = d2[q, order]
    return idx, dist


def transpose(idx):
    """(in_start (P + 1), in_edge (P K)): the valid edge ids stably sorted by target, -1 past the last"""
    P, K = idx.shape
    flat = idx.reshape(-1)
    edges = np.nonzero(flat >= 0)[0]
    order = edges[np.argsort(flat[edges], kind="stable")]
    in_edge = np.full(P * K, -1, np.int32)
    in_edge[:len(order)] = order
    in_start = np.zeros(P + 1, np.int32)
    in_start[1:] = np.cumsum(np.bincount(flat[edges], minlength=P))
    return in_start, in_edge


@functools.lru_cache(maxsize=None)
def knn_of(name, K):
    """the brute-force graph of a named cloud: (idx, dist2, in_start, in_edge), computed once"""
    if K < 16:  # a row's K best are the first K of its 16 best
        idx, dist = (np.ascontiguousarray(a[:, :K]) for a in knn_of(name, 16)[:2])
    else:
        x = cloud(name)
        idx, dist = knn_rows(x, K, np.arange(x.shape[0]))
    out = (idx, dist, *transpose(idx))
    for a in out:
        a.setflags(write=False)
    return out


def knn_fp64(x, K):
    """an independent fp64 brute force (the neighbour sets of a cloud without ties)"""
    x64 = np.asarray(x, np.float64)
    d = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, 1, kind="stable")[:, :K]


# ---- the loss -------------------------------------------------------------------------------------------------------
def isometry_torch(xa, xb, idx, weights=None):
    """1 / E sum over the valid edges of w (r(xb_i - xb_j) - r(xa_i - xa_j))^2 in xa's dtype, differentiable"""
    P, K = idx.shape
    valid = idx >= 0
    j = idx.clamp(min=0).long()
    E = P * min(K, P - 1)
    if E == 0:
        return (xa.sum() + xb.sum()) * 0
    ra = ((xa[:, None, :] - xa[j]).pow(2).sum(-1) + EPS).sqrt()
    rb = ((xb[:, None, :] - xb[j]).pow(2).sum(-1) + EPS).sqrt()
    w = valid.to(xa.dtype) if weights is None else weights.to(xa.dtype) * valid.to(xa.dtype)
    return (w * (rb - ra).pow(2)).sum() / E


def isometry_value_and_grads(xa, xb, idx, weights, dtype):
    """(value, dvalue/dxa, dvalue/dxb) of isometry_torch by autograd in `dtype`, on the inputs' device"""
    a = xa.detach().to(dtype).requires_grad_(True)
    b = xb.detach().to(dtype).requires_grad_(True)
    v = isometry_torch(a, b, idx, weights)
    ga, gb = torch.autograd.grad(v, (a, b))
    return v.detach(), ga, gb


def isometry_closed_form(xa, xb, idx, weights=None):
    """the issue's closed form in numpy fp64: (value, dxa, dxb), out-edge terms plus in-edge terms per node"""
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    P, K = idx.shape
    E = P * min(K, P - 1)
    ga, gb, value = np.zeros_like(xa), np.zeros_like(xb), 0.0
    for i in range(P):
        for k in range(K):
            j = idx[i, k]
            if j < 0:
                continue
            w = 1.0 if weights is None else float(weights[i, k])
            va, vb = xa[i] - xa[j], xb[i] - xb[j]
            ra, rb = np.sqrt(va @ va + EPS), np.sqrt(vb @ vb + EPS)
            delta = rb - ra
            value += w * delta * delta
            gb[i] += w * delta * vb / rb
            gb[j] -= w * delta * vb / rb
            ga[i] -= w * delta * va / ra
            ga[j] += w * delta * va / ra
    return value / E, 2.0 / E * ga, 2.0 / E * gb


def rel_err(t, t64):
    """max |T - T64| / max |T64| (0 when both vanish)"""
    t, t64 = t.detach().double().cpu(), t64.detach().double().cpu()
    scale = float(t64.abs().max()) if t64.numel() else 0.0
    err = float((t - t64).abs().max()) if t64.numel() else 0.0
    return err / scale if scale > 0 else err


def loss_inputs(name):
    """xa = the cloud, xb = xa + 0.05 * normal noise (CPU fp32 tensors)"""
    xa = torch.from_numpy(np.array(cloud(name)))
    g = torch.Generator().manual_seed(3)
    return xa, xa + 0.05 * torch.randn(xa.shape, generator=g)
