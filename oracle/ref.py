"""ctypes wrapper around the reference's own rasterizer and simple-knn, built for the host (oracle/ref_cpu).

TEST INFRASTRUCTURE ONLY, like oracle.py, and with its call shapes: `rasterize_forward`, `rasterize_backward`,
`mark_visible`, `knn_mean_dist`, and a state with `export()`.  Where oracle.py runs this project's C restatement of
forward.cu / backward.cu / rasterizer_impl.cu, this module runs those files themselves (oracle/ref_cpu/build_ref.py:
compiled by g++ against a CUDA-on-CPU shim, one block at a time, threads in rank order; single-threaded and
deterministic).  The library exists only where the reference checkout does; `available()` says whether it can be
used, and the tests that need it skip otherwise.

The `prefiltered` flag is not offered: the reference answers a filtered point with __trap(), which on the host
aborts the process.
"""
import ctypes
import os

import numpy as np

from oracle.ref_cpu import build_ref

_lib = None
_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def available():
    """True when oracle/_ref/libgs4d_ref.so exists, or the reference checkout does and the build succeeds."""
    if _lib is not None or os.path.exists(build_ref.LIB):
        return True
    try:
        return build_ref.build() is not None
    except Exception as e:  # a checkout that does not build is reported, then treated as absent
        print(f"oracle.ref: the reference host build failed: {e}", flush=True)
        return False


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if build_ref.reference_present():
        build_ref.build()  # no-op when up to date
    if not os.path.exists(build_ref.LIB):
        raise RuntimeError("oracle/_ref/libgs4d_ref.so is not built and there is no reference checkout to build it from")
    lib = ctypes.CDLL(build_ref.LIB)
    lib.gs4d_ref_forward.restype = ctypes.c_void_p
    lib.gs4d_ref_forward.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _f32p, _f32p,
        ctypes.c_float, _f32p, _f32p, _f32p, _f32p, _f32p, ctypes.c_float, ctypes.c_float, _f32p, _f32p, _i32p, _i32p]
    lib.gs4d_ref_backward.restype = None
    lib.gs4d_ref_backward.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, ctypes.c_float, _f32p, _f32p,
        _f32p, _f32p, _f32p, ctypes.c_float, ctypes.c_float, _i32p, _f32p,
        _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]
    lib.gs4d_ref_state_export.restype = None
    lib.gs4d_ref_state_export.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, _u8p, _u32p, _u32p, _u32p,
                                          _f32p, _u32p]
    lib.gs4d_ref_free.restype = None
    lib.gs4d_ref_free.argtypes = [ctypes.c_void_p]
    lib.gs4d_ref_mark_visible.restype = None
    lib.gs4d_ref_mark_visible.argtypes = [ctypes.c_int, _f32p, _f32p, _f32p, _u8p]
    lib.gs4d_ref_knn.restype = None
    lib.gs4d_ref_knn.argtypes = [ctypes.c_int, _f32p, _f32p]
    _lib = lib
    return lib


def _arr(a, dtype=np.float32):
    """None / empty -> NULL, as in oracle.py"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.size == 0:
        return None, None
    return a, a.ctypes.data_as({np.float32: _f32p, np.int32: _i32p}[dtype])


class RefState:
    """Owns the reference's three state chunks (geometry, binning, image) of one forward."""

    def __init__(self, handle, P, W, H, L):
        self.handle, self.P, self.W, self.H, self.L = handle, P, W, H, L

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.gs4d_ref_free(self.handle)
            self.handle = None

    def export(self):
        """OracleState.export()'s dict, read through the reference's own GeometryState / BinningState / ImageState
        fromChunk; `final_T` is the reference's accum_alpha, `clamped` packs its three bools per Gaussian into
        bits 0-2."""
        lib = _load()
        P, W, H, L = self.P, self.W, self.H, self.L
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        out = dict(
            depths=np.zeros(P, np.float32), means2D=np.zeros((P, 2), np.float32), cov3D=np.zeros((P, 6), np.float32),
            conic_opacity=np.zeros((P, 4), np.float32), rgb=np.zeros((P, 3), np.float32),
            clamped=np.zeros(P, np.uint8), tiles_touched=np.zeros(P, np.uint32),
            point_list=np.zeros(max(L, 1), np.uint32), ranges=np.zeros((tiles, 2), np.uint32),
            final_T=np.zeros((H, W), np.float32), n_contrib=np.zeros((H, W), np.uint32))
        p = lambda k, t: out[k].ctypes.data_as(t)
        lib.gs4d_ref_state_export(self.handle, p("depths", _f32p), p("means2D", _f32p), p("cov3D", _f32p),
                                  p("conic_opacity", _f32p), p("rgb", _f32p), p("clamped", _u8p),
                                  p("tiles_touched", _u32p), p("point_list", _u32p), p("ranges", _u32p),
                                  p("final_T", _f32p), p("n_contrib", _u32p))
        out["point_list"] = out["point_list"][:L]
        out["L"] = L
        return out


def rasterize_forward(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp,
                      viewmatrix, projmatrix, tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered=False):
    """oracle.rasterize_forward's arguments and results: (num_rendered, color (3,H,W), depth (1,H,W), radii (P,),
    state).  P = 0 returns without a call, as rasterize_points.cu does."""
    if prefiltered:
        raise NotImplementedError("prefiltered: the reference's __trap() would abort the process")
    lib = _load()
    means3D = np.ascontiguousarray(np.asarray(means3D, np.float32))
    P = means3D.shape[0]
    H, W = int(image_height), int(image_width)
    color = np.zeros((3, H, W), np.float32)
    depth = np.zeros((1, H, W), np.float32)
    radii = np.zeros(P, np.int32)
    if P == 0:
        return 0, color, depth, radii, None
    sh_a, sh_p = _arr(sh)
    M = sh_a.shape[1] if sh_a is not None else 0
    keep = [_arr(x) for x in (bg, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                              campos)]
    (_, bg_p), (_, cp_p), (_, op_p), (_, sc_p), (_, ro_p), (_, c3_p), (_, vm_p), (_, pm_p), (_, cam_p) = keep
    nr = ctypes.c_int(0)
    h = lib.gs4d_ref_forward(P, int(degree), M, bg_p, W, H, means3D.ctypes.data_as(_f32p), sh_p, cp_p, op_p, sc_p,
                             float(scale_modifier), ro_p, c3_p, vm_p, pm_p, cam_p, float(tanfovx), float(tanfovy),
                             color.ctypes.data_as(_f32p), depth.ctypes.data_as(_f32p), radii.ctypes.data_as(_i32p),
                             ctypes.byref(nr))
    return nr.value, color, depth, radii, RefState(h, P, W, H, nr.value)


def rasterize_backward(state, bg, means3D, radii, colors_precomp, scales, rotations, scale_modifier, cov3D_precomp,
                       viewmatrix, projmatrix, tanfovx, tanfovy, dL_dout_color, sh, degree, campos):
    """oracle.rasterize_backward's arguments and results: the 8-tuple (dL_dmeans2D, dL_dcolors, dL_dopacity,
    dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations), and dL_dconic (P, 4)."""
    lib = _load()
    means3D = np.ascontiguousarray(np.asarray(means3D, np.float32))
    P = means3D.shape[0]
    sh_a, sh_p = _arr(sh)
    M = sh_a.shape[1] if sh_a is not None else 0
    g = dict(
        dL_dmeans2D=np.zeros((P, 3), np.float32), dL_dconic=np.zeros((P, 4), np.float32),
        dL_dopacity=np.zeros((P, 1), np.float32), dL_dcolors=np.zeros((P, 3), np.float32),
        dL_dmeans3D=np.zeros((P, 3), np.float32), dL_dcov3D=np.zeros((P, 6), np.float32),
        dL_dsh=np.zeros((P, M, 3), np.float32), dL_dscales=np.zeros((P, 3), np.float32),
        dL_drotations=np.zeros((P, 4), np.float32))
    if P != 0:
        keep = [_arr(x) for x in (bg, colors_precomp, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                                  dL_dout_color)]
        (_, bg_p), (_, cp_p), (_, sc_p), (_, ro_p), (_, c3_p), (_, vm_p), (_, pm_p), (_, cam_p), (_, dl_p) = keep
        ra, rp = _arr(radii, np.int32)
        q = lambda k: g[k].ctypes.data_as(_f32p)
        lib.gs4d_ref_backward(
            state.handle, int(degree), M, bg_p, means3D.ctypes.data_as(_f32p), sh_p, cp_p, sc_p, float(scale_modifier),
            ro_p, c3_p, vm_p, pm_p, cam_p, float(tanfovx), float(tanfovy), rp, dl_p, q("dL_dmeans2D"), q("dL_dconic"),
            q("dL_dopacity"), q("dL_dcolors"), q("dL_dmeans3D"), q("dL_dcov3D"),
            g["dL_dsh"].ctypes.data_as(_f32p) if M > 0 else None, q("dL_dscales"), q("dL_drotations"))
    return (g["dL_dmeans2D"], g["dL_dcolors"], g["dL_dopacity"], g["dL_dmeans3D"], g["dL_dcov3D"], g["dL_dsh"],
            g["dL_dscales"], g["dL_drotations"]), g["dL_dconic"]


def mark_visible(means3D, viewmatrix, projmatrix):
    lib = _load()
    means3D = np.ascontiguousarray(np.asarray(means3D, np.float32))
    P = means3D.shape[0]
    out = np.zeros(P, np.uint8)
    if P:
        vm, vp = _arr(viewmatrix)
        pm, pp = _arr(projmatrix)
        lib.gs4d_ref_mark_visible(P, means3D.ctypes.data_as(_f32p), vp, pp, out.ctypes.data_as(_u8p))
    return out.astype(bool)


def knn_mean_dist(points):
    """SimpleKNN::knn of the reference: the mean squared distance to the three nearest other points."""
    lib = _load()
    pts = np.ascontiguousarray(np.asarray(points, np.float32))
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise RuntimeError("points must have dimensions (num_points, 3)")
    out = np.zeros(pts.shape[0], np.float32)
    if pts.shape[0]:
        lib.gs4d_ref_knn(pts.shape[0], pts.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    return out
