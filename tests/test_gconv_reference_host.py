"""The float64 reference, the operand generator and the plan restatements of the grouped-convolution case tables
(tests/gconv_cases.py) stand on their own, before a GPU is involved: the reference equals torch's float64 convolution on the CPU at
every case geometry, the generator's exactness conditions hold, and every case is in the regime its table row claims."""
import pytest
import torch
import torch.nn.functional as F

import gconv_cases as T

GEOMETRIES = sorted({(c["C"], c["H"], c["W"], c["stride"]) for c in T.BF16_CASES + T.F32_CASES + T.REFUSALS
                     if c["C"] % T.GROUPS == 0})
_ID = "C{}_{}x{}_s{}".format


@pytest.mark.parametrize("geo", GEOMETRIES, ids=[_ID(*g) for g in GEOMETRIES])
@pytest.mark.parametrize("prologue,centre", [(True, True), (False, False), (True, False), (False, True)])
def test_reference_is_float64_conv2d(geo, prologue, centre):
    """gconv_reference against F.conv2d in float64 on the CPU (exact on these integers: every sum is far below 2^53), B cut to 2"""
    C, H, W, stride = geo
    c = dict(C=C, H=H, W=W, stride=stride, B=2)
    t = T.gconv_inputs(c, 11 + C + 7 * H + W + stride, prologue=prologue, centre=centre)
    ref = T.gconv_reference(t["x"], t["scale"], t["shift"], t["w"], t["centre"], stride, T.GROUPS)
    act = t["x"].double()
    if prologue:
        act = torch.relu(act * t["scale"].double() + t["shift"].double())
    want = F.conv2d(act.permute(0, 3, 1, 2), t["w"].double(), None, stride, 1, 1, T.GROUPS).permute(0, 2, 3, 1)
    if centre:
        want = want - t["centre"].double()
    assert ref.dtype == torch.float64 and ref.shape == (2,) + T.out_hw(H, W, stride) + (C,)
    assert torch.equal(ref, want)
    # the generator's bound really bounds the result, and the result is a multiple of 0.5: exact in fp32 whatever the order
    assert float(ref.abs().max()) <= t["bound"] <= 3464
    assert torch.equal(ref * 2, (ref * 2).round())
    assert torch.equal(ref.float().double(), ref)


def test_reference_pads_after_the_activation():
    """a single pixel with shift > 0 everywhere: were the padding staged as relu(shift), the 1 x 1 map's output would see 9 taps"""
    C = 128
    x = torch.zeros(1, 1, 1, C)
    w = torch.ones(C, 4, 3, 3)
    ref = T.gconv_reference(x, torch.ones(C), torch.full((C,), 2.0), w, None, 1, T.GROUPS)
    assert torch.equal(ref, torch.full((1, 1, 1, C), 8.0, dtype=torch.float64))          # 4 channels x relu(0 + 2), centre tap only


@pytest.mark.parametrize("c", T.BF16_CASES, ids=[c["tag"] for c in T.BF16_CASES])
def test_bf16_cases_are_in_their_regime(c):
    p = T.bf16_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])
    Ho, Wo = T.out_hw(c["H"], c["W"], c["stride"])
    assert p["supported"], p
    assert p["staged"] <= 320 and p["TH"] * Wo <= 128 and p["TH"] <= 255
    if c["inst"] is not None:
        assert p["inst"] == c["inst"], p
    for k in ("grid", "items", "trips", "TH", "staged", "partial"):
        if k in c:
            assert p[{"grid": "grid_x"}.get(k, k)] == c[k], (k, p)
    if "n_out" in c:
        assert p["TH"] * Wo == c["n_out"], p
    if c.get("multi"):
        assert p["grid_x"] < p["items"], p
    if "multi" in c and not c["multi"]:
        assert p["grid_x"] == p["items"], p
    if "xcd" in c:
        assert (p["grid_x"] % 8 == 0) == c["xcd"], p
    if c.get("odd_s2"):
        assert c["stride"] == 2 and c["H"] % 2 and c["W"] % 2
    if c.get("trips") == 3:
        assert p["items"] % p["grid_x"] != 0                                     # the last trip is a partial one


def test_tables_reach_every_instantiation_and_regime():
    plans = [(c, T.bf16_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])) for c in T.BF16_CASES]
    assert {p["inst"] for _, p in plans} == T.ALL_INSTANTIATIONS
    assert len(T.ALL_INSTANTIATIONS) == 16
    for wide in (False, True):                                                   # each regime in both kernel variants
        mine = [(c, p) for c, p in plans if p["inst"][0] == wide]
        assert any(p["grid_x"] < p["items"] and p["grid_x"] % 8 == 0 for _, p in mine)
        assert any(p["partial"] for _, p in mine)
        assert any(c["stride"] == 2 and c["H"] % 2 and c["W"] % 2 and c["H"] > 1 for c, _ in mine)
    assert any(p["grid_x"] < p["items"] and p["partial"] for _, p in plans)      # a partial band on a second trip
    for tag in T.VARIATION_TAGS + T.ACCUMULATE_TAGS:
        T.by_tag(tag)


@pytest.mark.parametrize("c", T.REFUSALS, ids=[c["tag"] for c in T.REFUSALS])
def test_refused_shapes_are_outside_the_plan(c):
    p = T.bf16_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])
    if c.get("rows_short"):
        assert p["supported"] and p["grid_x"] > 1
    else:
        assert not p["supported"], p
    if c["tag"] == "row_321_pixels":
        assert p["staged"] == 321


@pytest.mark.parametrize("c", T.F32_CASES, ids=[c["tag"] for c in T.F32_CASES])
def test_f32_cases_are_in_their_regime(c):
    p = T.f32_plan(c["B"], c["H"], c["W"], c["C"], c["stride"], aligned=not c.get("misaligned"))
    assert p["tiled"] == (not c.get("misaligned")), p
    if c.get("misaligned"):                                                      # a shape the tiled kernel would take, were x aligned
        assert T.f32_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])["tiled"]
    if c.get("second_trip"):
        assert p["items"] > p["gx"] == 1024 // (c["C"] // 64), p
    if c.get("partial"):
        assert p["partial"], p
    if c.get("ragged"):
        assert p["n_out"] % 64 != 0 or p["last_n_out"] % 64 != 0, p


def test_f32_second_trip_cases_cover_every_group_width():
    assert {T.f32_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])["cg"] for c in T.F32_CASES if c.get("second_trip")} == {4, 8, 16, 32}


def test_generator_bounds_hold_for_every_case():
    """the asserts inside gconv_inputs run for every case (B cut to 2); a third of the channels has a positive shift"""
    for c in T.BF16_CASES + T.F32_CASES:
        for prologue, centre in ((True, True), (False, False)):
            t = T.gconv_inputs(c, 5, prologue=prologue, centre=centre, B=2)
            assert t["bound"] * 2 < 2 ** 24
            if prologue:
                assert int((t["shift"] > 0).sum()) * 3 >= c["C"]
                assert float(t["shift"].min()) >= -2 and float(t["shift"].max()) <= 2
            if centre:
                assert float(t["centre"].abs().max()) <= 8
