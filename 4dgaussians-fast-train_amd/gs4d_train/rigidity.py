"""Local rigidity: an exact K-NN graph of the canonical Gaussians and the fused local-isometry term over it.

Neighbouring Gaussians should keep their mutual distances as the scene deforms (Dynamic 3D Gaussians' isometry term,
SC-GS's ARAP term): over the valid edges e = (i, k), j = idx[i, k], of a K-NN graph,

    loss = 1 / E * sum_e w_e * (r(xb_i - xb_j) - r(xa_i - xa_j))^2,   r(v) = sqrt(v.v + 1e-12),   E = P min(K, P - 1).

The graph is simple_knn._C.knn_graph (gs4d_knn_graph, csrc/knn.hip: the exact K nearest others and the transposed
graph); the value and both gradients come from one fused pass (gs4d_isometry_loss_grad, csrc/rigidity.hip) whose
sums run in an order fixed by the graph: no float atomics, the same bits in two calls.  The reference has no such
term; everything here is opt-in (train_step(rigidity=...), opt.lambda_rigid).
"""
import torch

from .render import _time_float, _time_value

__all__ = ["KnnGraph", "build_graph", "isometry_loss", "isometry_loss_and_grad", "isometry_between_times", "Rigidity"]


class KnnGraph:
    """idx, dist2 (P, K), in_start (P + 1), in_edge (P K) as simple_knn._C.knn_graph returns them, K, P and the
    per-edge weights (P, K) or None (= 1)."""

    def __init__(self, idx, dist2, in_start, in_edge, weights=None):
        self.idx, self.dist2, self.in_start, self.in_edge, self.weights = idx, dist2, in_start, in_edge, weights
        self.P, self.K = int(idx.shape[0]), int(idx.shape[1])


def build_graph(points, K=8, weight_lambda=None):
    """The exact K-NN graph of `points` (P, 3), detached.  weight_lambda: weights = exp(-weight_lambda * dist2), 0 in
    the empty slots (Dynamic 3D Gaussians uses 2000 in its units); None (the default): no weights, every edge 1."""
    from simple_knn import _C as knn
    idx, dist2, in_start, in_edge = knn.knn_graph(points.detach(), int(K))
    weights = None
    if weight_lambda is not None:
        weights = torch.where(idx >= 0, torch.exp(-float(weight_lambda) * dist2), torch.zeros_like(dist2))
    return KnnGraph(idx, dist2, in_start, in_edge, weights)


def _check(xa, xb, graph):
    for name, x in (("xa", xa), ("xb", xb)):
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError(f"isometry_loss: {name} must be (P, 3), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"isometry_loss: {name} must be float32, got {x.dtype}")
    if xa.shape != xb.shape:
        raise ValueError(f"isometry_loss: xa {tuple(xa.shape)} and xb {tuple(xb.shape)} differ in shape")
    if xa.device != xb.device or xa.device != graph.idx.device:
        raise ValueError(f"isometry_loss: xa ({xa.device}), xb ({xb.device}) and the graph ({graph.idx.device}) must "
                         "be on one device")
    if not xa.is_cuda:
        raise ValueError("isometry_loss: the positions must be HIP (GPU) tensors; there is no CPU path")
    if graph.P != xa.shape[0]:
        raise ValueError(f"isometry_loss: the graph was built for {graph.P} rows, the positions have {xa.shape[0]}")


def _call(xa, xb, graph, scale, want_a, want_b):
    from . import _C
    return _C.isometry_loss_grad(graph.idx, graph.in_start, graph.in_edge, graph.weights, xa.detach().contiguous(),
                                 xb.detach().contiguous(), float(scale), bool(want_a), bool(want_b))


class _Isometry(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xa, xb, graph):
        # the value and the gradients of the sides that require grad in the one pass; backward scales them
        value, ga, gb = _call(xa, xb, graph, 1.0, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.save_for_backward(*[g for g in (ga, gb) if g is not None])
        ctx.have = (ga is not None, gb is not None)
        return value

    @staticmethod
    def backward(ctx, dvalue):
        saved = list(ctx.saved_tensors)
        ga = saved.pop(0) * dvalue if ctx.have[0] else None
        gb = saved.pop(0) * dvalue if ctx.have[1] else None
        return ga, gb, None


def isometry_loss(xa, xb, graph):
    """The isometry term between the position sets xa and xb (P, 3) over `graph`, differentiable to both."""
    _check(xa, xb, graph)
    return _Isometry.apply(xa, xb, graph)


def isometry_loss_and_grad(xa, xb, graph, scale=1.0):
    """(detached scale * loss, its gradient to xa, its gradient to xb) in one pass, without an autograd node: what
    (scale * isometry_loss(xa, xb, graph)).backward() deposits, for the fused train step."""
    _check(xa, xb, graph)
    return _call(xa, xb, graph, scale, True, True)


def _means_at(pc, t):
    """the deformed means at time t by a positions-only pass (flow.flow_rows' pass): the field and the position
    head as plain layers"""
    xyz = pc.get_xyz
    net = pc._deformation.deformation_net
    if net.args.no_dx:
        return xyz
    tt = _time_value(_time_float(t), xyz.device).expand(xyz.shape[0], 1)
    return xyz + net.pos_deform(net.feature_out(net.grid(xyz, tt)))


def isometry_between_times(pc, t0, t1, graph):
    """The isometry term between the deformed means at times t0 and t1 (each a positions-only pass through the
    deformation), for loops that constrain time to time instead of canonical to time."""
    return isometry_loss(_means_at(pc, t0), _means_at(pc, t1), graph)


class Rigidity:
    """The K-NN graph of a model's canonical means, kept between steps.  graph_for(gaussians, iteration) builds it on
    the detached get_xyz and rebuilds it when the rows have changed since the build (surgery.apply bumps
    gaussians.row_generation; the row count is compared as well) or `refresh_interval` iterations have passed."""

    def __init__(self, K=8, weight_lambda=None, refresh_interval=100):
        self.K, self.weight_lambda, self.refresh_interval = int(K), weight_lambda, int(refresh_interval)
        self.graph = None
        self.builds = 0
        self._key = None
        self._built_at = None

    def graph_for(self, gaussians, iteration):
        xyz = gaussians.get_xyz
        key = (id(gaussians), getattr(gaussians, "row_generation", 0), int(xyz.shape[0]), xyz.device)
        if self.graph is None or key != self._key or iteration - self._built_at >= self.refresh_interval \
                or iteration < self._built_at:
            self.graph = build_graph(xyz.detach(), self.K, self.weight_lambda)
            self._key, self._built_at = key, iteration
            self.builds += 1
        return self.graph
