"""The side-stream suite's parts that need no GPU (tests/stream_cases.py): every bound entry point has a case or
a reasoned exclusion, the bitwise comparison tells one flipped bit, the case builders give a real and a decoy input
set of the same shapes, and the delay arithmetic."""
import math

import pytest
import torch

import stream_cases as SC


# ---- coverage -------------------------------------------------------------------------------------------------------
def test_every_bound_entry_point_has_a_case_or_a_reason():
    names = SC.bound_names()
    assert len(set(names)) >= 56 and "distCUDA2" in names and "hexplane_reg_accumulate" in names  # multi-line defs too
    bound = set(names)
    unaccounted = sorted(bound - set(SC.CASE_TABLE) - set(SC.EXCLUDED))
    assert not unaccounted, f"no side-stream case and no exclusion for {unaccounted}"
    both = sorted(set(SC.CASE_TABLE) & set(SC.EXCLUDED))
    assert not both, f"both a case and an exclusion: {both}"
    stale = sorted((set(SC.EXCLUDED) | set(SC.CASE_TABLE)) - bound)
    assert not stale, f"names that no module binds: {stale}"
    for name, reason in SC.EXCLUDED.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3, f"{name}: an exclusion needs its reason"
    print(f"[streams] {len(bound)} bound names: {len(SC.CASE_TABLE)} with cases ({len(SC.CASES)} cases), "
          f"{len(SC.EXCLUDED)} excluded", flush=True)


def test_the_parser_reads_multi_line_defs(tmp_path, monkeypatch):
    (tmp_path / "a.cpp").write_text('m.def("one", &f);\n    m.def(\n        "two", &g, py::arg("x"));\n// m.def(name)\n')
    monkeypatch.setattr(SC, "CSRC", str(tmp_path))
    monkeypatch.setattr(SC, "GLUE", ("a.cpp",))
    assert SC.bound_names() == ["one", "two"]


def test_the_named_subsets_are_cases():
    for name in SC.SECOND_STREAM + SC.SECOND_DEVICE:
        assert name in SC.CASES, name
    for c in SC.CASES.values():
        assert c.exact or (c.bar is not None and c.bar > 0), c.name


# ---- the comparison helper ------------------------------------------------------------------------------------------
def test_one_flipped_mantissa_bit_is_a_mismatch():
    a = torch.linspace(-3, 3, 1001)
    b = a.clone()
    assert SC.first_difference([a], [b]) is None
    b.view(torch.int32)[500] ^= 1
    d = SC.first_difference([a], [b])
    assert d is not None and "1 of 1001" in d and "index 500" in d
    h = a.to(torch.bfloat16)
    g = h.clone()
    g.view(torch.int16)[7] ^= 1
    assert SC.first_difference([h], [h.clone()]) is None and SC.first_difference([h], [g]) is not None


def test_shape_dtype_and_count_are_compared():
    a = torch.zeros(6)
    assert SC.first_difference([a], [a.reshape(2, 3)]) is not None
    assert SC.first_difference([a], [a.to(torch.int32)]) is not None
    assert SC.first_difference([a], [a, a]) is not None
    assert SC.first_difference([], []) is None
    assert SC.first_difference([torch.zeros(0, 3)], [torch.zeros(0, 3)]) is None
    t, f = torch.tensor([True, False]), torch.tensor([True, True])
    assert SC.first_difference([t], [t.clone()]) is None and SC.first_difference([t], [f]) is not None


def test_signed_zeros_differ_and_equal_nan_bits_agree():
    assert SC.first_difference([torch.tensor([0.0])], [torch.tensor([-0.0])]) is not None
    nan = torch.tensor([float("nan"), 1.0])
    assert SC.first_difference([nan], [nan.clone()]) is None
    other = nan.clone()
    other.view(torch.int32)[0] ^= 1  # another NaN payload
    assert math.isnan(float(other[0])) and SC.first_difference([nan], [other]) is not None


def test_the_bar_of_inexact_cases():
    a = torch.tensor([1.0, 100.0])
    assert SC.within_bar([a], [a + 5e-4], 1e-5) is None          # 5e-4 <= 1e-5 * 100
    assert SC.within_bar([a], [a + 5e-3], 1e-5) is not None
    assert SC.within_bar([a], [a.reshape(1, 2)], 1e-5) is not None
    assert SC.within_bar([torch.tensor([float("nan")])], [torch.tensor([1.0])], 1e-5) is not None


# ---- the case builders ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES) + ["control"])
def test_real_and_decoy_share_shapes_and_differ(name):
    case = SC.CONTROL_GOOD if name == "control" else SC.CASES[name]
    real, decoy, again = case.make(SC.SEED), case.make(SC.SEED + 1), case.make(SC.SEED)
    assert list(real) == list(decoy) and len(real) >= 1
    for k in real:
        assert real[k].device.type == "cpu" and not real[k].requires_grad
        assert real[k].dtype == decoy[k].dtype and real[k].shape == decoy[k].shape, k
        assert torch.equal(SC.bits(real[k]), SC.bits(again[k])), f"{k}: the builder is not a function of its seed"
        if real[k].is_floating_point():
            assert bool(torch.isfinite(real[k]).all()) and bool(torch.isfinite(decoy[k]).all()), k
    key = SC.probe_key(real, decoy)
    differing = [k for k in real if not torch.equal(SC.bits(real[k]), SC.bits(decoy[k]))]
    assert key == differing[0] and real[key].is_floating_point()
    with pytest.raises(SC.HarnessInvalid):
        SC.probe_key(real, again)


def test_index_inputs_stay_in_range_for_both_seeds():
    """a decoy is another valid input: a kernel that reads it computes a wrong value, never out of bounds"""
    for seed in (SC.SEED, SC.SEED + 1):
        t = SC.CASES["rows_assemble"].make(seed)
        assert t["keep"].dtype == t["append"].dtype == torch.int32
        assert int(t["keep"].min()) >= 0 and int(t["keep"].max()) < SC.ROWS_P and t["keep"].numel() == 700
        assert int(t["append"].min()) >= 0 and int(t["append"].max()) < SC.ROWS_P and t["append"].numel() == SC.ROWS_A
        d = SC.CASES["densify_stats"].make(seed)
        assert d["vis"].dtype == torch.bool and d["radii"].dtype == torch.int32 and int(d["radii"].min()) >= 0
    sizes = SC.hex_sizes()
    assert len(sizes) == 12 and sizes[0] == (64, 64) and sizes[2] == (64, 25) and sizes[6] == (128, 128)
    assert any(n % 4 for n in (math.prod(s) for s in SC.ADAM_SHAPES)) and len(SC.ADAM_SHAPES) == 3


# ---- the delay arithmetic -------------------------------------------------------------------------------------------
def test_delays_follow_the_measurements():
    d_side, d_null = SC.delays_ms(0.02, 0.3)                 # quick call: the floors
    assert d_side == SC.D_SIDE_FLOOR_MS and d_null == d_side + SC.D_NULL_ROOM_MS
    d_side, d_null = SC.delays_ms(3.0, 7.5)                  # slow call: ten times what was measured
    assert d_side == 30.0 and d_null == 30.0 + 75.0
    for enq, t in ((0.0, 0.0), (0.4, 0.1), (12.0, 40.0)):
        s, n = SC.delays_ms(enq, t)
        assert s >= 10 * enq and n >= s + 10 * t and s > 0 and n > s
    for bad in ((-1.0, 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(ValueError):
            SC.delays_ms(*bad)


def test_cycles_round_up():
    assert SC.cycles_for(2.0, 1000.0) == 2000
    assert SC.cycles_for(0.00001, 1000.0) == 1                 # never a zero-length spin
    assert SC.cycles_for(1.0001, 1000.0) == 1001
    assert isinstance(SC.cycles_for(3.0, 123456.7), int)
    with pytest.raises(ValueError):
        SC.cycles_for(1.0, 0.0)
