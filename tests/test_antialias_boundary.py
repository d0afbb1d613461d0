"""CPU tests of the opt-in antialiased rasterization's boundary (no GPU calls): the three C entries exist and
report argument errors as status codes, the Python surface defaults to off, and on every scene of
tests/antialias_scenes.py the margins hold that let tests/test_antialias_gpu.py compare every element -- all of it
from the fp64 restatement (tests/antialias_refs.py) and the fp32 oracle run on the folded plain problem (opacities
fl32(o s), s from fp64), never from the code under test.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import antialias_refs as AAR
import antialias_scenes as AS
import torch_restatement as TR
from gpu_helpers import o_bounds
from test_depth_grad_gpu import needed_floor
from test_rule_branches_boundary import CLAMP_MARGIN, TERM_MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "4dgaussians-fast-train_amd", "diff_gaussian_rasterization", "libgs4d.so")
FLOOR_MARGIN = 0.5   # |r / 2.5e-5 - 1| of every listed Gaussian
MIN_FLOORED_BLENDING = 8
MIN_CLAMPED = 5      # aa_clampcam: clamped Gaussians that still overlap the image


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libgs4d.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.gs4d_last_error.restype = ctypes.c_char_p
    return L


def _decl(text, name):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\s*\(([^;]*)\);", text, flags=re.S)
    assert m, f"{name} is not declared (with its comment)"
    return m.group(1), [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]


def test_header_declares_and_library_exports_the_entries(lib):
    text = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    m = re.search(r"int gs4d_forward_ex\s*\(([^;]*)\);", text)
    fwd = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    comment, params = _decl(text, "gs4d_forward_aa")
    assert params == fwd + ["int antialiasing"]
    assert "2.5e-5" in comment and "sqrt" in comment and "radii" in comment and "num_rendered" in comment
    _, bwd = _decl(text, "gs4d_backward_absgrad")
    comment, params = _decl(text, "gs4d_backward_aa")
    assert params == bwd + ["const float *opacities", "int antialiasing"]
    assert "D1^2" in comment and "denom2inv" in comment and "NULL" in comment
    comment, params = _decl(text, "gs4d_debug_effective_opacity")
    assert params == ["int P", "const char *geometry_buffer", "float *out", "void *stream"]
    assert "unspecified" in comment
    for name in ("gs4d_forward_aa", "gs4d_backward_aa", "gs4d_debug_effective_opacity"):
        assert hasattr(lib, name), name


def _bwd_args(P, R, dL_dpix, opacities, aa):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [i(P), i(0), i(0), i(R), null, i(16), i(16), null, null, null, null, f(1.0), null, null, null, null, null,
            f(1.0), f(1.0), null, null, null, null, dL_dpix, null, null] + [null] * 9 + [null] + \
        [null, null, i(0), null, i(0), opacities, i(aa)]


def _fwd_args(P, W, aa, num_rendered):
    null = ctypes.c_void_p(0)
    i, f = ctypes.c_int, ctypes.c_float
    return [null] * 6 + [i(P), i(0), i(0), null, i(W), i(16)] + [null] * 5 + [f(1.0)] + [null] * 5 + \
        [f(1.0), f(1.0), i(0), null, null, null, i(0), null, num_rendered, i(0), i(aa)]


def test_argument_errors_are_status_codes(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    # antialiasing needs the raw opacities; without it they are not looked at
    assert lib.gs4d_backward_aa(*_bwd_args(4, 0, some, null, 1)) == 1
    assert lib.gs4d_last_error().startswith(b"backward_aa")
    assert lib.gs4d_backward_aa(*_bwd_args(4, 0, some, null, 0)) == 1   # ... but the buffers are still missing
    assert lib.gs4d_last_error().startswith(b"backward:")
    for P, R in ((-1, 0), (4, -1)):
        assert lib.gs4d_backward_aa(*_bwd_args(P, R, some, some, 1)) == 1
    for aa in (0, 1):  # P == 0 succeeds at once
        assert lib.gs4d_backward_aa(*_bwd_args(0, 0, null, null, aa)) == 0
    nr = ctypes.c_int(-1)
    for aa in (0, 1):
        assert lib.gs4d_forward_aa(*_fwd_args(0, 16, aa, ctypes.byref(nr))) == 0 and nr.value == 0
        assert lib.gs4d_forward_aa(*_fwd_args(-1, 16, aa, ctypes.byref(nr))) == 1
        assert lib.gs4d_forward_aa(*_fwd_args(4, 0, aa, ctypes.byref(nr))) == 1
        assert lib.gs4d_forward_aa(*_fwd_args(4, 16, aa, ctypes.byref(nr))) == 1   # missing inputs
    assert lib.gs4d_debug_effective_opacity(ctypes.c_int(0), null, null, null) == 0
    assert lib.gs4d_debug_effective_opacity(ctypes.c_int(-1), some, some, null) == 1
    assert lib.gs4d_debug_effective_opacity(ctypes.c_int(4), null, some, null) == 1
    assert lib.gs4d_debug_effective_opacity(ctypes.c_int(4), some, null, null) == 1
    assert lib.gs4d_last_error().startswith(b"debug_effective_opacity")


def test_python_surface_is_opt_in_and_not_a_fourth_axis():
    import diff_gaussian_rasterization as dgr
    from gs4d_train import config, infer
    from gs4d_train.render import render
    for name in ("rasterize_gaussians_aa", "rasterize_gaussians_backward_aa", "debug_effective_opacity"):
        assert hasattr(dgr._C, name), name
    e = torch.zeros(4, 4)
    st = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, e, e, 0, torch.zeros(3), False, False)
    assert len(dgr.GaussianRasterizationSettings._fields) == 12
    assert inspect.signature(dgr.GaussianRasterizer.__init__).parameters["antialiasing"].default is False
    assert dgr.GaussianRasterizer(st).antialiasing is False
    assert dgr.GaussianRasterizer(st, antialiasing=True).antialiasing is True
    for fn in (dgr.rasterize_gaussians, render, infer.render_view, infer.render_set, infer.evaluate):
        assert inspect.signature(fn).parameters["antialiasing"].default is False, fn
    assert config.optimization_params().antialiasing is False
    assert len(dgr._FUNCTIONS) == 8 and len(dgr.__all__) == 11


def test_switch_travels_as_a_tenth_input_only_when_on(monkeypatch):
    """with the switch off the Function gets today's nine arguments; on, the same Function gets a tenth"""
    import diff_gaussian_rasterization as dgr
    seen = []
    for fn in set(dgr._FUNCTIONS.values()):
        monkeypatch.setattr(fn, "apply", staticmethod(lambda *a, _n=fn.__name__: seen.append((_n, len(a), a[9:]))))
    for key, fn in dgr._FUNCTIONS.items():
        for aa in (False, True):
            seen.clear()
            dgr.rasterize_gaussians(*range(9), depth_grad=key[0], alpha=key[1], absgrad=key[2], antialiasing=aa)
            assert seen == [(fn.__name__, 10, (True,))] if aa else seen == [(fn.__name__, 9, ())]


def test_train_step_passes_the_switch_to_render_fn():
    """opt.antialiasing reaches render_fn as antialiasing=True on every view, and not at all when it is off"""
    import test_absgrad_boundary as TA

    class Renderer(TA._Renderer):
        def __call__(self, cam, pc, debug, bg, stage="coarse", **kw):
            self.seen.append(dict(kw))
            kw.pop("antialiasing", None)
            return super().__call__(cam, pc, debug, bg, stage=stage, **kw)

    views = TA._views(2)
    calls = {}
    for key, over in (("on", dict(antialiasing=True)), ("off", dict(antialiasing=False)), ("none", {}),
                      ("both", dict(antialiasing=True, densify_absgrad=True))):
        r = Renderer()
        r.seen = []
        TA._step(views, r, **over)
        calls[key] = r.seen
    assert calls["on"] == [{"antialiasing": True}] * 2
    assert calls["off"] == [{}] * 2 and calls["none"] == [{}] * 2
    assert calls["both"] == [{"absgrad": True, "antialiasing": True}] * 2


# ---- the scenes ------------------------------------------------------------------------------------------------
def preconditions(O, sc, r, g_c):
    """Assert the conditions under which every element of the scene can be compared (also used to look for seeds)"""
    name, s, ref, ex = sc["name"], sc["s"], r["ref"], r["export"]
    b = o_bounds(O, r["fold"], r["state"], r["radii"], g_c, colors=sc["colors"], cov3D=sc["cov3D"], use_sh=sc["use_sh"])
    assert int((np.asarray(b["gflag"]) != 0).sum()) == 0 and int((np.asarray(b["pflag"]) != 0).sum()) == 0
    assert ref["near_threshold"] == 0
    assert np.array_equal(ref["n_contrib"], ex["n_contrib"])
    listed, vis = ref["listed"], r["radii"] > 0
    assert listed.sum() >= 50 and not (listed & ~vis).any()
    fdist = np.abs(r["r64"] / AAR.AA_FLOOR - 1.0)
    assert fdist[listed].min() >= FLOOR_MARGIN, fdist[listed].min()
    if name == "aa_floor":
        rows = np.arange(len(vis)) % AS.FLOOR_EVERY == 0
        assert np.array_equal(r["floored"], rows) and r["r64"][rows].max() < 0.1 * AAR.AA_FLOOR
        assert int((ref["blends"] & rows).sum()) >= MIN_FLOORED_BLENDING, int((ref["blends"] & rows).sum())
    else:
        assert not r["floored"].any()
    if name == "aa_clampcam":
        assert int((ref["clamped"] & vis).sum()) >= MIN_CLAMPED, int((ref["clamped"] & vis).sum())
        assert np.abs(s["viewmatrix"].reshape(4, 4)[:3, :3] - np.eye(3)).max() > 0.1
    else:
        assert ref["n_clamped"] == 0
    assert ref["clamp_margin"] >= CLAMP_MARGIN, ref["clamp_margin"]
    assert not ref["nonpd"][vis].any() and ref["n_power_rejected"] == 0
    assert ref["clamp099"] == 0 and ref["n_terminated"] == 0 and ref["term_margin"] >= TERM_MARGIN


@pytest.mark.parametrize("name", AS.NAMES)
def test_scene_preconditions(oracle, name):
    sc, r = AS.scene(name), AS.reference(oracle, name)
    ref = r["ref"]
    sv = r["s64"][ref["listed"]]
    print(f"[aa-scenes] {name}: listed {int(ref['listed'].sum())}, s {sv.min():.3f}-{sv.max():.3f} median "
          f"{np.median(sv):.3f}, floored {int(r['floored'].sum())} (blending "
          f"{int((ref['blends'] & r['floored']).sum())}), clamped {ref['n_clamped']} (margin "
          f"{ref['clamp_margin']:.2e}), kappa max {r['kappa'][ref['listed']].max():.1f}, min T {ref['min_T']:.2e}",
          flush=True)
    preconditions(oracle, sc, r, AS.upstream(oracle, name, "color")[0])


def test_s_ranges_on_seeds_0_and_1():
    """the ranges the two scales were chosen for, over all P Gaussians of seeds 0 and 1: aa_small's s spans about
    0.04-0.92 around a median of 0.42, aa_mid's 0.15-0.98 around 0.74 (within the slack below, P = 200 sampling
    the tails thinly), and neither has a Gaussian at the floor"""
    for make, lo, hi, med in ((AS._small, 0.04, 0.92, 0.42), (AS._mid, 0.15, 0.98, 0.74)):
        for seed in (0, 1):
            s64, r64, floored, _ = AAR.factor(make(seed))
            assert not floored.any()
            assert s64.min() < 2.5 * lo and s64.max() > hi - 0.08 and abs(np.median(s64) - med) < 0.06, \
                (seed, s64.min(), s64.max(), np.median(s64))


@pytest.mark.parametrize("name", AS.NAMES)
def test_restatement_is_the_plain_one_with_the_folded_opacity(oracle, name):
    """The conic and the images of antialias_refs equal torch_restatement's on the same scene with opacities o s
    (fp64, not rounded): the restatement differs from the tested one in s and nothing else.  And the gradient with
    respect to the raw opacity is s times the folded one's."""
    sc, r = AS.scene(name), AS.reference(oracle, name)
    s, ref, ex = sc["s"], r["ref"], r["export"]
    fold64 = dict(s)
    fold64["opacities"] = s["opacities"].astype(np.float64) * r["s64"][:, None]
    plain = TR.forward_autograd(fold64, ex["point_list"], ex["ranges"], s["sh_degree"],
                                use_precomp_colors=sc["colors"] is not None, colors=sc["colors"], cov3D=sc["cov3D"])
    for k in ("color", "depth", "Tfinal"):
        assert torch.allclose(ref[k], plain[k], rtol=1e-12, atol=1e-14), k
    g_a = torch.autograd.grad(ref["color"].sum(), ref["opac"], retain_graph=True)[0][:, 0].numpy()
    g_p = torch.autograd.grad(plain["color"].sum(), plain["opac"], retain_graph=True)[0][:, 0].numpy()
    np.testing.assert_allclose(g_a, g_p * r["s64"], rtol=1e-10, atol=1e-14)
    if name == "aa_floor":  # the floored rows: a non-zero dL/do and nothing through s
        rows = r["floored"] & ref["blends"]
        assert np.abs(g_a[rows]).min() > 0
        np.testing.assert_array_equal(r["s64"][r["floored"]], np.sqrt(AAR.AA_FLOOR))


@pytest.mark.parametrize("name", AS.NAMES)
def test_oracle_floor_on_the_folded_problem(oracle, name):
    """F_oracle, the floor the fp32 oracle's colour backward needs against fp64 on the folded plain problem (the GPU
    test's bar is built from it), and the oracle's images against fp64 within the bars of tests/test_oracle.py"""
    from test_rule_branches_gpu import _pairs
    got, want, radii, plain = AS.oracle_floor_pairs(oracle, name)
    r = AS.reference(oracle, name)
    np.testing.assert_allclose(r["color"], plain["color"].detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(r["depth"], plain["depth"].detach().numpy(), atol=2e-5)
    f_oracle = needed_floor(_pairs(got, want, radii))
    print(f"[aa-oracle] {name}: F_oracle = {f_oracle:.3e}", flush=True)
    assert f_oracle < 2e-4
