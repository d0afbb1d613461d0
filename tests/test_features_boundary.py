"""CPU tests of the feature-rendering boundary (no GPU calls): gs4d_features_forward / gs4d_features_backward are
declared and exported and refuse bad input with their status codes; the Python surface exists, is opt-in and raises
the errors it documents; and the two properties of tests/feature_refs.py's references that tests/test_features_gpu.py
rests on: Reference B with three channels is forward_autograd's colour over a zero background, and its gradients at
C = 7 are the sums of its groups of three channels (the linearity the composition, Reference A, is built on)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import depth_scenes as DS
import feature_refs as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    return L


def _params(text, name):
    m = re.search(r"int " + name + r"\s*\(([^;]*)\);", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_two_entries(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert _params(text, "gs4d_features_forward") == [
        "int P", "int C", "int width", "int height", "int num_rendered", "const char *geometry_buffer",
        "const char *binning_buffer", "const char *image_buffer", "const float *features", "float *out_image",
        "gs4d_alloc_fn scratch_alloc", "void *scratch_ctx", "void *stream"]
    back = _params(text, "gs4d_features_backward")
    assert back[:5] == ["int P", "int C", "int num_rendered", "int width", "int height"]
    for p in ("const float *features", "const float *dL_dfeature_image", "float *dL_dfeatures", "float *dL_dmean2D",
              "float *dL_dopacity", "float *dL_dmean3D", "float *dL_dcov3D", "float *dL_dscale", "float *dL_drot",
              "const float *opacities", "int antialiasing", "gs4d_alloc_fn scratch_alloc"):
        assert p in back, p
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int gs4d_feature_chunk", text, flags=re.S)
    comment = re.sub(r"[\s*]+", " ", m.group(1))
    assert "no background" in comment and "bit for bit" in comment and "float atomics" in comment
    assert all(hasattr(lib, n) for n in ("gs4d_features_forward", "gs4d_features_backward", "gs4d_feature_chunk"))
    assert lib.gs4d_feature_chunk() >= 1


def _ptrs():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)


def _forward(lib, P=4, C=3, W=16, H=16, R=8, geom=True, binning=True, image=True, feats=True, out=True):
    buf, some, null = _ptrs()
    p = lambda on: some if on else null
    i = ctypes.c_int
    st = lib.gs4d_features_forward(i(P), i(C), i(W), i(H), i(R), p(geom), p(binning), p(image), p(feats), p(out),
                                   ALLOC(), null, null)
    return st, lib.gs4d_last_error()


def _backward(lib, P=4, C=3, R=8, W=16, H=16, geom=True, binning=True, image=True, feats=True, grad=True, dfeat=True,
              dmean2D=True, dopacity=True, means3D=True, alloc="null"):
    buf, some, null = _ptrs()
    p = lambda on: some if on else null
    calls = []

    def returns_null(ctx, n):
        calls.append(n)
        return None
    cb = ALLOC(returns_null) if alloc == "null" else ALLOC()
    i, f = ctypes.c_int, ctypes.c_float
    st = lib.gs4d_features_backward(
        i(P), i(C), i(R), i(W), i(H), p(means3D), some, f(1.0), some, null, some, some, f(0.5), f(0.5), null, p(geom),
        p(binning), p(image), p(feats), p(grad), p(dfeat), p(dmean2D), p(dopacity), some, some, some, some, cb, null,
        null, i(0), null, i(0))
    return st, lib.gs4d_last_error(), calls


def test_argument_errors_are_status_codes(lib):
    for kw in [dict(P=-1), dict(C=0), dict(C=-2), dict(W=0), dict(H=0), dict(R=-1), dict(geom=False),
               dict(binning=False), dict(image=False), dict(feats=False), dict(out=False)]:
        st, msg = _forward(lib, **kw)
        assert st == 1 and msg.startswith(b"features:"), (kw, st, msg)  # GS4D_ERR_ARG
    assert _forward(lib, P=0, W=0, H=0, geom=False, binning=False, image=False, feats=False, out=False)[0] == 0
    assert _forward(lib, P=0, C=0)[0] == 1  # C < 1 is an error whatever P
    for kw in [dict(P=-1), dict(C=0), dict(W=0), dict(H=-1), dict(R=-1), dict(geom=False), dict(binning=False),
               dict(image=False), dict(feats=False), dict(grad=False), dict(dfeat=False), dict(dopacity=False),
               dict(means3D=False), dict(alloc=None)]:
        st, msg, calls = _backward(lib, **kw)
        assert st == 1 and msg.startswith(b"features:"), (kw, st, msg)
        assert calls == [], kw  # refused before the scratch is asked for
    # the allocator returning NULL is GS4D_ERR_ALLOC; it was asked for R records of FEATURE_CHUNK + 12 floats and more
    K = lib.gs4d_feature_chunk()
    st, msg, calls = _backward(lib)
    assert st == 2 and msg.startswith(b"features:") and len(calls) == 1 and calls[0] >= 8 * 4 * (K + 12)
    # without the geometry outputs the records are the K floats alone
    st, msg, few = _backward(lib, dmean2D=False, dopacity=False, means3D=False)
    assert st == 2 and len(few) == 1 and 8 * 4 * K <= few[0] < calls[0]
    assert _backward(lib, P=0, W=0, H=0, geom=False, image=False, feats=False, grad=False, dfeat=False, alloc=None)[0] == 0


def test_python_surface_exists_and_is_opt_in():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import flow, infer, render, train
    C = dgr._C
    assert callable(C.rasterize_features) and callable(C.rasterize_features_backward)
    assert isinstance(C.FEATURE_CHUNK, int) and C.FEATURE_CHUNK >= 1
    for fn in (dgr.rasterize_gaussians, dgr.GaussianRasterizer.forward, render.render, infer.render_view):
        par = inspect.signature(fn).parameters
        assert "features" in par and par["features"].default is None, fn
    assert list(inspect.signature(flow.render_flow).parameters) == ["camera", "pc", "bg", "dt", "stage", "render_kwargs"]
    assert len(dgr._FUNCTIONS) == 8  # the features ride the existing Functions
    src = inspect.getsource(train.train_step)
    assert "features" not in src and "flow" not in src
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    m3, m2, op = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 1)
    kw = dict(means3D=m3, means2D=m2, opacities=op, shs=torch.zeros(5, 16, 3), scales=torch.zeros(5, 3),
              rotations=torch.zeros(5, 4))
    bad = [torch.zeros(5), torch.zeros(5, 2, 1), torch.zeros(5, 2, dtype=torch.float64), torch.zeros(4, 2),
           torch.zeros(5, 0), torch.zeros(5, 2, device="meta"), np.zeros((5, 2), np.float32)]
    for f in bad:
        with pytest.raises(ValueError):
            dgr.GaussianRasterizer(st)(features=f, **kw)
    with pytest.raises(ValueError):
        dgr.GaussianRasterizer(st, camera_grad=True)(features=torch.zeros(5, 2), **kw)
    with pytest.raises(RuntimeError):  # no CPU path
        C.rasterize_features(torch.zeros(5, 2), torch.zeros(64, dtype=torch.uint8), 4,
                             torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), 5, 8, 8)


def _reference_b(oracle, name):
    sc = DS.scene(name)
    ref = DS.reference(oracle, name)
    return sc, ref, FR.restatement(sc["s"], ref["export"]["point_list"], ref["export"]["ranges"])


def test_reference_b_with_three_channels_is_the_colour_over_a_zero_background(oracle):
    from torch_restatement import forward_autograd
    sc, ref, r = _reference_b(oracle, "small0")
    s = dict(sc["s"])
    s["bg"] = np.zeros(3, np.float32)
    P = len(s["means3D"])
    f = FR.features_of(P, 3, 7)
    want = forward_autograd(s, ref["export"]["point_list"], ref["export"]["ranges"], s["sh_degree"],
                            use_precomp_colors=True, colors=f)["color"]
    got = FR.features_image(r, torch.tensor(f, dtype=torch.float64))
    want = want.detach()
    assert float(want.abs().max()) > 0.1 and torch.equal(got, want)


def test_reference_b_gradients_are_the_sums_of_their_groups(oracle):
    sc, ref, r = _reference_b(oracle, "small0")
    s = sc["s"]
    P, H, W = len(s["means3D"]), s["H"], s["W"]
    f = FR.features_of(P, 7, 8)
    g = FR.upstream_normal(7, H, W, 9)
    full = FR.restatement_grads(r, torch.tensor(f, dtype=torch.float64, requires_grad=True), g)
    parts = [FR.restatement_grads(r, torch.tensor(f[:, a:a + 3], dtype=torch.float64, requires_grad=True), g[a:a + 3])
             for a in (0, 3, 6)]
    for k in ("means2D", "opacities", "means3D", "scales", "rotations"):
        total = sum(p[k] for p in parts)
        scale = np.abs(full[k]).max()
        assert scale > 0 and np.abs(total - full[k]).max() <= 1e-12 * scale, k  # fp64 re-association only
    assert np.allclose(np.concatenate([p["features"] for p in parts], 1), full["features"], rtol=1e-12, atol=0)
