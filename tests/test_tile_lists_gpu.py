"""GPU tests of the rasterizer's two discrete stages -- the per-tile (depth bits, id) sort and the exact tile culling
-- on the lists themselves (gs4d_debug_tile_lists), with no tolerance: against a numpy lexsort, the oracle's point_list
and the fp64 alpha test of tests/tile_list_scenes.py.  One forward per scene; no pair, tile or pixel is left out.
tests/test_tile_lists_boundary.py asserts on the CPU that the scenes are what these comparisons assume.

The sort's six paths by run length (1 | 2-64 | 65-128 | 129-256 in render.hip; 257-2048 and > 2048 in binning.hip)
are walked at their edges by the stack scenes; the binning's variants (counting with 4, 8 or 16 keys per lane, radix)
by a 129x129-tile grid and by GS4D_BINNING / GS4D_COUNT_MIN_ITEMS in child processes, whose lists and images must
equal the default path's to the bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tile_list_scenes as TL
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu
_RUNS = {}


def _C():
    import diff_gaussian_rasterization as dgr
    return dgr._C


def run(name):
    """the scene's forward and lists, made once"""
    if name not in _RUNS:
        _RUNS[name] = TL.gpu_lists(_C(), name)
    return _RUNS[name]


def _common(name, oracle):
    """structure and order of the lists of `name`, every scene; returns (fwd, lists)"""
    s = TL.scene(name)["s"]
    P, T = len(s["means3D"]), ((s["W"] + 15) // 16) * ((s["H"] + 15) // 16)
    fwd, lists = run(name)
    assert TL.structure_errors(lists, T, fwd[0], P) == []
    assert TL.order_errors(lists, s["means3D"][:, 2]) == []  # identity view: the view depth is z
    if oracle is not None:
        o = TL.oracle_run(oracle, name)
        assert fwd[0] == o["nr"]
        assert TL.oracle_order_errors(lists, o["export"], P) == []
    return fwd, lists


@pytest.mark.parametrize("name", list(TL.STACKS) + list(TL.TOTALS))
def test_stack_lists_equal_lexsort(oracle, name):
    s = TL.scene(name)["s"]
    T = s["gx"] * s["gy"]
    fwd, lists = _common(name, oracle if name in TL.ORACLE_STACKS or name in TL.TOTALS else None)
    want_ranges, want_gid = TL.lexsort_lists(s["tile_of"], s["z"], T)
    assert fwd[0] == lists["n"] == len(want_gid)  # nothing culled: both halves of every pair are reachable
    r = np.asarray(lists["ranges"], np.int64)
    assert np.array_equal(r[:, 1] - r[:, 0], s["lengths_by_tile"])
    assert np.array_equal(r, want_ranges)
    bad = np.nonzero(lists["gid"] != want_gid)[0]
    tiles = TL.tiles_of_positions(r, len(want_gid))
    assert len(bad) == 0, (f"{len(bad)} positions differ from lexsort, in tiles of length "
                           f"{sorted(set(s['lengths_by_tile'][tiles[bad]].tolist()))}")
    assert np.all(lists["reach"] == 3)


@pytest.mark.parametrize("name", list(TL.AUDITS))
def test_culling_drops_no_reachable_pair(oracle, name):
    s = TL.scene(name)["s"]
    fwd, lists = _common(name, oracle)
    ref = TL.reach_of(oracle, name)
    err, wasted = TL.culling_errors(lists, ref, len(s["means3D"]))
    st = TL.reach_stats(ref)
    # a performance figure, not asserted: pairs the continuous-rectangle bound keeps although no pixel centre of
    # either half reaches 1/255
    print(f"[tile-lists] {name}: L = {fwd[0]}, L' = {lists['n']}, reachable pairs {st['reachable']}, emitted but "
          f"unreachable {wasted:.4f} of L', one-half pairs {st['one_half']}, not positive definite {st['nonpd']}",
          flush=True)
    assert err == []


@pytest.mark.parametrize("name", ["7x4_random", "7x4_ties"])
def test_consumers_of_every_list_length(oracle, name):
    """forward + backward parity at oracle/parity.py's default shares: blend lists of every length through the
    batch and refill edges, the backward reading the order the forward wrote back"""
    _check(_C(), oracle, TL.scene(name)["s"], torch.device("cuda:0"))


def test_two_forwards_give_the_same_lists():
    a = TL.gpu_lists(_C(), "32x9_ties")
    b = TL.gpu_lists(_C(), "32x9_ties")
    for k in ("ranges", "gid", "reach", "slot", "depth"):  # `order` is arbitrary among tiles of one length
        assert np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)), k
    assert a[1]["n"] == b[1]["n"] and torch.equal(a[0][1], b[0][1])


_VARIANT_SCENES = ["7x4_ties", "sh3000"]
_CHILD = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import diff_gaussian_rasterization as dgr
import tile_list_scenes as TL
for name in sys.argv[4:]:
    print("digest", name, *TL.digests(*TL.gpu_lists(dgr._C, name)))
"""


@pytest.mark.parametrize("var,value", [("GS4D_BINNING", "radix"), ("GS4D_COUNT_MIN_ITEMS", "4"),
                                        ("GS4D_COUNT_MIN_ITEMS", "16")])
def test_binning_variants_give_the_default_lists(var, value):
    """The variables are read once per process, so each setting runs in a fresh child (one at a time)."""
    assert var not in os.environ
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "4dgaussians-fast-train_amd"), os.path.join(root, "tests")]
    r = subprocess.run([sys.executable, "-c", _CHILD, *paths, *_VARIANT_SCENES], capture_output=True, text=True,
                       timeout=55, env=dict(os.environ, **{var: value}))
    assert r.returncode == 0, r.stderr[-2000:]
    got = {ln.split()[1]: ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("digest ")}
    for name in _VARIANT_SCENES:
        want = list(TL.digests(*run(name)))
        print(f"[tile-lists] {var}={value} {name}: lists {got[name][0][:16]} image {got[name][1][:16]}; default "
              f"{want[0][:16]} {want[1][:16]}", flush=True)
        assert got[name] == want and len(want[0]) == 64
