"""The K-NN graph and the isometry term without a GPU: the C ABI's declarations, exports and status codes (through
ctypes: every refusal comes before any launch), and the references of tests/rigidity_refs.py against independent
restatements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rigidity_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
OK, ERR_ARG, ERR_ALLOC = 0, 1, 2
ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.gs4d_knn_graph.argtypes = [i, i, p, p, p, p, p, ALLOC_FN, p, p]
    L.gs4d_isometry_loss_grad.argtypes = [i, i, p, p, p, p, p, p, f, p, p, p, ALLOC_FN, p, p]
    return L


class Allocator:
    """counts its calls; returns NULL (or a host buffer nobody may touch: the call under test must fail first)"""

    def __init__(self):
        self.calls = 0
        self.fn = ALLOC_FN(self._alloc)

    def _alloc(self, ctx, n):
        self.calls += 1
        return None


NULL_ALLOC = ctypes.cast(None, ALLOC_FN)
PTR = 0x1000  # a non-NULL pointer that is never dereferenced: the refusals come before any launch


def test_headers_declare_the_entries():
    with open(os.path.join(ROOT, "include", "gs4d.h")) as f:
        assert re.search(r"\bint gs4d_knn_graph\(int P, int K, const float \*points", f.read())
    with open(os.path.join(ROOT, "include", "gs4d_train.h")) as f:
        assert re.search(r"\bint gs4d_isometry_loss_grad\(int P, int K, const int32_t \*nbr_idx", f.read())


def test_library_exports_the_entries(lib):
    assert lib.gs4d_knn_graph and lib.gs4d_isometry_loss_grad


def _graph(lib, P, K, alloc, points=PTR, idx=PTR, dist=PTR, start=PTR, edge=PTR):
    return lib.gs4d_knn_graph(P, K, points, idx, dist, start, edge, alloc, None, None)


def _iso(lib, P, K, alloc, idx=PTR, start=PTR, edge=PTR, xa=PTR, xb=PTR, value=PTR):
    return lib.gs4d_isometry_loss_grad(P, K, idx, start, edge, None, xa, xb, 1.0, value, None, None, alloc, None, None)


@pytest.mark.parametrize("call,prefix", [(_graph, b"knn_graph:"), (_iso, b"isometry:")], ids=["knn_graph", "isometry"])
def test_status_codes(lib, call, prefix):
    a = Allocator()
    assert call(lib, 0, 8, a.fn) == OK  # P == 0: at once
    for P, K in ((100, 0), (100, 17), (-1, 8)):
        assert call(lib, P, K, a.fn) == ERR_ARG
        assert lib.gs4d_last_error().startswith(prefix)
    assert call(lib, 100, 8, NULL_ALLOC) == ERR_ARG and lib.gs4d_last_error().startswith(prefix)
    names = ("points", "idx", "dist", "start", "edge") if call is _graph else ("idx", "start", "edge", "xa", "xb", "value")
    for name in names:
        assert call(lib, 100, 8, a.fn, **{name: None}) == ERR_ARG, name
        assert lib.gs4d_last_error().startswith(prefix)
    assert a.calls == 0  # every refusal above came before the allocator was asked
    assert call(lib, 100, 8, a.fn) == ERR_ALLOC and lib.gs4d_last_error().startswith(prefix)
    assert a.calls == 1


def test_brute_force_agrees_with_fp64_where_no_tie_exists():
    idx = RR.knn_of("gauss", 8)[0]
    assert np.array_equal(idx, RR.knn_fp64(RR.cloud("gauss"), 8))
    # and its own invariants: ascending, no self, no repeats; the transpose lists every edge once under its target
    idx, dist, in_start, in_edge = RR.knn_of("hub", 8)
    P, K = idx.shape
    assert (np.diff(dist, axis=1) >= 0).all() and (idx != np.arange(P)[:, None]).all()
    assert all(len(set(r)) == K for r in idx)
    assert in_start[0] == 0 and in_start[-1] == P * K and sorted(in_edge) == list(range(P * K))
    for t in (0, 7, 1500, P - 1):
        e = in_edge[in_start[t]:in_start[t + 1]]
        assert (np.diff(e) > 0).all() and (idx.reshape(-1)[e] == t).all()
    assert in_start[P] - in_start[P - 1] == 0  # the far point is the neighbour of nobody


def test_cloud_table():
    """the clouds' properties the GPU tests rest on: ties at the K-th place, high in-degree, in-degree 0"""
    stats = {}
    for name in RR.LOSS_CLOUDS:
        idx16, d16 = RR.knn_of(name, 16)[:2]
        indeg = np.diff(RR.knn_of(name, 8)[2])
        stats[name] = (int(indeg.max()), int((indeg == 0).sum()), float((d16[:, 7] == d16[:, 8]).mean()))
    print(stats)
    assert stats["gauss"][2] == 0.0 and stats["gauss"][1] > 0
    assert stats["lattice"][2] == 1.0 and stats["lattice"][1] == 0
    assert stats["hub"][0] >= 300 and stats["hub"][1] >= 290 and 0.1 < stats["hub"][2] < 0.25


def test_fp64_graph_matches_the_closed_form():
    P, K = 65, 8
    x = np.random.default_rng(2).normal(size=(P, 3)).astype(np.float32)
    idx = RR.knn_rows(x, K, np.arange(P))[0]
    g = torch.Generator().manual_seed(4)
    xa = torch.from_numpy(x)
    xb = xa + 0.05 * torch.randn(P, 3, generator=g)
    w = torch.rand(P, K, generator=g, dtype=torch.float64)
    for weights in (None, w):
        v, ga, gb = RR.isometry_value_and_grads(xa, xb, torch.from_numpy(idx), weights, torch.float64)
        cv, cga, cgb = RR.isometry_closed_form(xa.numpy(), xb.numpy(), idx, None if weights is None else w.numpy())
        assert abs(float(v) - cv) <= 1e-13 * abs(cv)
        np.testing.assert_allclose(ga.numpy(), cga, rtol=0, atol=1e-13 * np.abs(cga).max())
        np.testing.assert_allclose(gb.numpy(), cgb, rtol=0, atol=1e-13 * np.abs(cgb).max())


def test_fp32_twin_error_on_the_test_inputs():
    """e_u of the unfused fp32 formulation on the CPU, for the record (the GPU tests measure it on the GPU)"""
    for name in RR.LOSS_CLOUDS:
        xa, xb = RR.loss_inputs(name)
        idx = torch.from_numpy(np.array(RR.knn_of(name, 8)[0]))
        r64 = RR.isometry_value_and_grads(xa, xb, idx, None, torch.float64)
        r32 = RR.isometry_value_and_grads(xa, xb, idx, None, torch.float32)
        e_u = [RR.rel_err(a, b) for a, b in zip(r32, r64)]
        print(name, ["%.2e" % e for e in e_u])
        assert max(e_u) < 1e-5
