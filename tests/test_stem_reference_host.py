"""The float64 references, the operand generators and the launcher restatements of tests/stem_cases.py stand on their own, before a
GPU is involved: the references equal torch's float64 convolution / max-pool on the CPU, every case of the tables is in the regime
its row claims (both sides of every boundary included), and the exactness bounds the GPU tests rely on hold for every case."""
import pytest
import torch
import torch.nn.functional as F

import stem_cases as T

F64 = torch.float64


def _ids(cases):
    return [c["tag"] for c in cases]


def _claims(c, p, keys):
    for k in keys:
        if k in c:
            assert p[k] == c[k], (c["tag"], k, p)


# ---- references -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (1, 36, 72), (2, 6, 20), (1, 4, 44), (3, 2, 4)])
@pytest.mark.parametrize("centre", [True, False])
def test_stem_reference_is_float64_conv2d(B, H, W, centre):
    x, w, cen = T.stem_inputs(B, H, W, 3 + H + W, centre=centre)
    ref = T.stem_reference(x, w, cen)
    want = F.conv2d(x.double(), w.double(), None, 2, 3).permute(0, 2, 3, 1)
    if centre:
        want = want - cen.double()
    assert ref.dtype == F64 and ref.shape == (B, H // 2, W // 2, 64)
    assert torch.equal(ref, want)
    assert float(ref.abs().max()) <= 1184 and torch.equal(ref * 2, (ref * 2).round()) and torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 8), (1, 15, 17, 16), (3, 14, 9, 8), (1, 1, 5, 8), (1, 2, 2, 8), (2, 7, 7, 24)])
def test_maxpool_reference_is_float64_max_pool2d(B, H, W, C):
    x = T.int_activations((B, H, W, C), H * W, "cpu")
    scale, shift = T.pool_affine(C, seed=1)
    ref = T.maxpool_reference(x, scale, shift)
    act = torch.relu(x.double() * scale.double() + shift.double())
    want = F.max_pool2d(act.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(ref, want)
    assert float(act.min()) == 0 and bool((x.double() * scale.double() + shift.double() < 0).any())      # the ReLU matters
    # every value is a multiple of 1/8 below 2^12: exact in fp32, so the fp32 kernel must return it and the bf16 one its rounding
    assert torch.equal(ref * 8, (ref * 8).round()) and float(ref.max()) < 4096


def test_stem_pool_reference_is_the_composition():
    x, w, cen = T.stem_inputs(2, 12, 24, 5)
    scale, shift = T.pool_affine(64, seed=2)
    raw = (F.conv2d(x.double(), w.double(), None, 2, 3) - cen.double()[None, :, None, None]).float().to(torch.bfloat16)
    act = torch.relu(raw.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None])
    want = F.max_pool2d(act, 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(T.stem_pool_reference(x, w, cen, scale, shift), want)
    assert float(want.max()) > 256                                  # the final bf16 rounding is a real one


def test_bn_add_relu_reference_is_plain_torch():
    raw, idn = T.int_activations((5, 24), 1, "cpu"), T.int_activations((5, 24), 2, "cpu")
    (s1, b1), (s2, b2) = T.pool_affine(24, 0), T.pool_affine(24, 3)
    assert torch.equal(T.bn_add_relu_reference(raw, s1, b1, idn, None, None), torch.relu(raw.double() * s1 + b1 + idn.double()))
    assert torch.equal(T.bn_add_relu_reference(raw, s1, b1, idn, s2, b2),
                       torch.relu(raw.double() * s1 + b1 + (idn.double() * s2 + b2)))


def test_affine_pairs_differ_in_every_channel():
    for C in (4, 8, 24, 40, 72, 256, 2048):
        for seed in (0, 3):
            scale, shift = T.pool_affine(C, seed)
            assert len({(float(a), float(b)) for a, b in zip(scale, shift)}) == C
            assert torch.equal(shift * 8, (shift * 8).round()) and set(scale.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}


def test_bn_finalize_reference_is_batch_norm():
    """bn_finalize_reference on the column statistics of a random tensor against torch's own train-mode batch_norm in float64"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(500, 17, generator=g).double() * 2 + 1
    stats = torch.stack([x.sum(dim=0), (x * x).sum(dim=0)]).float()[None]
    gamma, beta = torch.rand(17, generator=g) + 0.5, torch.randn(17, generator=g)
    rm, rv = torch.randn(17, generator=g), torch.rand(17, generator=g) + 0.5
    r = T.bn_finalize_reference(stats, 500, gamma, beta, rm, rv, 0.1, 1e-5, None)
    rm64, rv64 = rm.double(), rv.double()
    y = F.batch_norm(x, rm64, rv64, gamma.double(), beta.double(), True, 0.1, 1e-5)
    assert float((x * r["scale"] + r["shift"] - y).abs().max()) < 1e-5            # (the statistics were rounded to fp32 once)
    assert float((r["running_mean"] - rm64).abs().max()) < 1e-5 and float((r["running_var"] - rv64).abs().max()) < 1e-5


@pytest.mark.parametrize("rows", T.FINALIZE_ROWS)
def test_finalize_exact_inputs_add_up(rows):
    for C in (1, 17):
        for count in T.FINALIZE_COUNTS:
            for neg in (False, True):
                t = T.finalize_exact_inputs(rows, C, count, rows + C + count, "cpu", negative_var=neg)
                s = t["stats"].double().sum(dim=0)
                assert torch.equal(s[0] / count, t["mean"])
                raw_var = s[1] / count - t["mean"] * t["mean"]
                assert torch.equal(raw_var, torch.full_like(raw_var, -2.0 ** -6) if neg else t["var"])
                r = T.bn_finalize_reference(t["stats"], count, t["gamma"], t["beta"], t["rm"], t["rv"], 0.5, 0.25, t["centre"])
                root = torch.sqrt(r["var"] + 0.25)
                assert torch.equal(torch.log2(root), torch.log2(root).round())      # var + eps is a power of four
                for k in ("scale", "shift", "running_mean"):                        # dyadic: fp32 holds them exactly
                    assert torch.equal(r[k].float().double(), r[k]), k
                if neg:
                    assert torch.equal(r["var"], torch.zeros_like(r["var"])) and torch.equal(r["scale"], t["gamma"].double() * 2)


# ---- regimes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.BF16_STEM_CASES, ids=_ids(T.BF16_STEM_CASES))
def test_bf16_stem_cases_are_in_their_regime(c):
    p = T.bf16_stem_plan(c["B"], c["H"], c["W"])
    assert p["supported"], p
    _claims(c, p, ("bands", "items", "grid", "xcd", "trips", "mtiles", "partial_band", "partial_tile"))
    assert p["mtiles"] <= 8                                             # the patch row holds 8 tiles x 16 pixels + 3 + slack


def test_bf16_stem_table_reaches_every_regime():
    plans = {c["tag"]: T.bf16_stem_plan(c["B"], c["H"], c["W"]) for c in T.BF16_STEM_CASES}
    assert any(p["trips"] == 2 and p["xcd"] for p in plans.values())
    assert any(p["trips"] == 1 and not p["xcd"] and p["items"] > 1 for p in plans.values())
    assert any(p["partial_band"] and p["partial_tile"] for p in plans.values())
    assert any(p["mtiles"] < 4 for p in plans.values()) and any(c["H"] != c["W"] for c in T.BF16_STEM_CASES)
    assert T.bf16_stem_supported(32, 256) and not T.bf16_stem_supported(32, 260)       # both sides of the width limit
    for r in T.BF16_STEM_REFUSALS:
        assert not T.bf16_stem_supported(r["H"], r["W"]), r


def test_item_order_is_a_permutation_with_residue_classes():
    """first_item (the kernels' ``bx``) is a permutation of the workgroups, so the items of a workgroup are one residue class
    modulo the grid whatever the order: item_workgroup"""
    for grid in (15, 8, 512, 256, 260, 9):
        firsts = [T.first_item(b, grid) for b in range(grid)]
        assert sorted(firsts) == list(range(grid))
        assert all(T.item_workgroup(f + grid, grid) == f for f in firsts)
    assert [T.first_item(b, 16) for b in range(4)] == [0, 2, 4, 6] and T.first_item(8, 16) == 1


@pytest.mark.parametrize("c", T.F32_STEM_CASES, ids=_ids(T.F32_STEM_CASES))
def test_f32_stem_cases_are_in_their_regime(c):
    p = T.f32_stem_plan(c["B"], c["H"], c["W"])
    _claims(c, p, ("tiled", "TH", "items", "grid", "trips", "partial_band"))
    if p["tiled"]:
        assert p["lds"] <= 150 * 1024


def test_f32_stem_boundaries():
    """the widths at which the fp32 launcher changes its mind: 21 (W + 6) <= 28928 floats of band fit beside the weights"""
    assert T.f32_stem_plan(1, 6, 1370)["tiled"] and T.f32_stem_plan(1, 6, 1370)["TH"] == 1
    assert not T.f32_stem_plan(1, 6, 1372)["tiled"]
    assert T.f32_stem_plan(1, 20, 452)["TH"] == 8 and T.f32_stem_plan(1, 20, 454)["TH"] == 7           # the band starts to shrink
    assert T.f32_stem_plan(4, 224, 224)["TH"] == 8
    assert T.f32_stem_plan(128, 128, 32)["grid"] == 1024 == T.f32_stem_plan(128, 128, 32)["items"]      # the last single-trip batch


@pytest.mark.parametrize("c", T.STEM_POOL_CASES, ids=_ids(T.STEM_POOL_CASES))
def test_stem_pool_cases_are_in_their_regime(c):
    p = T.stem_pool_plan(c["B"], c["H"], c["W"], c.get("cus", 256))
    assert p["supported"], p
    _claims(c, p, ("Hp", "items", "trips", "xcd", "mtiles", "partial_band", "tile_past_row"))


def test_stem_pool_boundaries():
    assert T.stem_pool_supported(16, 252) and not T.stem_pool_supported(16, 256)
    for W in range(4, 256, 4):                                          # the widths whose last tile reaches the band row's end
        assert T.stem_pool_plan(1, 16, W, 256)["tile_past_row"] == (228 <= W <= 252), W
    assert T.stem_pool_plan(64, 32, 228, 256)["trips"] == 1 and T.stem_pool_plan(65, 32, 228, 256)["trips"] == 2


def test_pooling_and_affine_grids():
    assert T.maxpool_plan(64, 64, 64, 512)["total"] == 8192 * 256 and T.maxpool_plan(64, 64, 64, 512)["trips"] == 1
    p = T.maxpool_plan(*T.MAXPOOL_PAST_CAP)
    assert p["grid"] == 8192 and p["trips"] == 2
    assert T.maxpool_plan(256, 112, 112, 64)["trips"] > 1               # the B = 256 stem map runs in this regime
    for shape in T.MAXPOOL_SHAPES:
        assert T.maxpool_plan(*shape)["trips"] == 1 and shape[3] % 8 == 0
    for dt, epc in (("f32", 4), ("bf16", 8)):
        mults = {T.affine_plan(1, C, epc)["mult"] for C in T.affine_channels(epc)}      # cc / gcd(cc, 256): the rounding unit
        assert {1, 3, 5, 9} <= mults, mults
        for C in T.affine_channels(epc):
            for rows in T.AFFINE_ROWS:
                p = T.affine_plan(rows, C, epc)
                assert (p["grid"] * 256) % p["cc"] == 0 and p["grid"] <= 16384 + p["mult"]
        for C in T.affine_channels(epc)[1:4]:                               # a rounded grid on which threads take several chunks
            p = T.affine_plan(1100, C, epc)
            assert p["rounded"] and p["several"] and (p["capped"] * 256) % p["cc"] != 0, p
        rows, C = T.AFFINE_PAST_CAP[dt]
        p = T.affine_plan(rows, C, epc)
        assert p["capped"] == 16384 and p["rounded"] and p["mult"] == 3, p
        assert p["total"] > 16384 * 1024 and p["trips"] == 2 and p["tail"] and p["tail_both"], p
    assert T.affine_plan(256 * 3136, 256, 8)["trips"] > 1               # layer 1 of the B = 256 workload: past the cap
    B, HW, C = T.AVGPOOL_PAST_CAP
    assert T.avgpool_plan(B, C)["grid"] == 4096 and T.avgpool_plan(B, C)["trips"] == 2
    assert T.avgpool_plan(512, 2048)["trips"] == 1


def test_col_stats_rows_and_blocks():
    assert [T.col_stats_rows(r) for r in T.COL_STATS_ROWS] == [1, 1, 1, 4, 256]
    assert T.col_stats_rows(65536) == 256 and T.col_stats_rows(65537) == 256 and T.col_stats_rows(0) == 1
    blk = T.col_stats_block(65536 + 7, 256)
    assert int(blk[1024]) == 0 and int(blk[1023]) == 255 and int(blk[65536 + 6]) == 1      # second trips, and a 65th for two blocks
    assert torch.bincount(blk, minlength=256).tolist()[:3] == [260, 259, 256]


# ---- exactness bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [True, False])
@pytest.mark.parametrize("c", T.BF16_STEM_CASES, ids=_ids(T.BF16_STEM_CASES))
def test_bf16_stem_outputs_and_partials_are_exact(c, centre):
    """|y| < 2^24 halves, outputs beyond 256 (bf16 keeps even integers only there: a real rounding, with ties), and every workgroup's
    fp32 partial below 2^24 units in every channel"""
    x, w, cen = T.stem_inputs(c["B"], c["H"], c["W"], 1, centre=centre)
    ref = T.stem_reference(x, w, cen)
    exp = ref.float().to(torch.bfloat16)
    assert float(ref.abs().max()) * 2 < 2 ** 24 and float(ref.abs().max()) > 256
    assert not torch.equal(exp.double(), ref)
    assert bool(((ref.abs() > 256) & (ref % 2 == 1)).any())             # odd integers above 256: ties
    s, q = T.stem_stats_bound(exp, T.bf16_stem_plan(c["B"], c["H"], c["W"]))
    print(f"{c['tag']} centre={centre}: largest workgroup partial {s:.0f} halves, {q:.0f} quanta of squares")
    assert s < 2 ** 24 and q < 2 ** 24


@pytest.mark.parametrize("c", T.F32_STEM_CASES, ids=_ids(T.F32_STEM_CASES))
def test_f32_stem_outputs_and_partials_are_exact(c):
    x, w, cen = T.stem_inputs(c["B"], c["H"], c["W"], 2, centre=True)
    ref = T.stem_reference(x, w, cen)
    assert float(ref.abs().max()) * 2 < 2 ** 24 and torch.equal(ref.float().double(), ref)
    y = ref.reshape(-1, 64)
    s, q = T.col_stats_bound(y, T.col_stats_rows(y.shape[0]))
    assert s < 2 ** 24 and q < 2 ** 24, (s, q)
