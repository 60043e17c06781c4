"""The float64 references, the operand generators and the launcher restatements of tests/trunk_bwd_cases.py stand on their own,
before a GPU is involved: the references equal torch autograd in float64 on the CPU (train-mode batch_norm plain, with relu and with
relu(. + identity); max_pool2d with return_indices; conv2d gradients grouped, strided and the 7x7/2 stem; the data gradient of a
grouped 3x3 conv as a conv2d with the flipped weight), every case of the tables is in the regime its row claims, the restatements
agree with cvcl_bn_bwd_partial_rows, and every exact case IS exact: each float64 intermediate the kernel holds in fp32 is
representable in fp32.  A case that is not exact fails here, not on the GPU."""
import pytest
import torch
import torch.nn.functional as F

from multimodal import _hip as H

import trunk_bwd_cases as T

F64 = torch.float64


def _ids(cases):
    return [c["tag"] for c in cases]


# ---- references against autograd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rows,C", [(7, 4), (64, 8), (33, 24)])
def test_bn_bwd_reference_is_batch_norm_autograd(mode, rows, C):
    """random float64 data with its true batch statistics: dx, dgamma, dbeta and the identity's gradient g are those of
    F.batch_norm(train), plain, under relu, and under relu(. + identity)"""
    g = torch.Generator().manual_seed(rows * 3 + C + mode)
    x = (torch.randn(rows, C, generator=g, dtype=F64) * 2 + 1).requires_grad_()
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_()
    idn = torch.randn(rows, C, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(rows, C, generator=g, dtype=F64)
    eps = 1e-5
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
    out = y if mode == 0 else torch.relu(y) if mode == 1 else torch.relu(y + idn)
    (out * dy).sum().backward()
    with torch.no_grad():
        mean = x.mean(dim=0)
        rstd = 1.0 / torch.sqrt(x.var(dim=0, unbiased=False) + eps)
        scale = gamma * rstd
        shift = beta - mean * scale
        r = T.bn_bwd_reference(mode, x, out, dy, scale, shift, mean, rstd, gamma)
    for got, want in ((r["dx"], x.grad), (r["dgamma"], gamma.grad), (r["dbeta"], beta.grad)):
        assert float((got - want).abs().max()) < 1e-10
    if mode == 2:
        assert torch.equal(r["g"], idn.grad)
    assert torch.equal(r["inner"], r["k2"] * x.detach() + r["k3"]) and torch.equal(r["k3"], r["a0"] - r["k2mean"])


@pytest.mark.parametrize("shape", T.MAXPOOL_IDX_SHAPES, ids=["x".join(map(str, s)) for s in T.MAXPOOL_IDX_SHAPES])
def test_maxpool_idx_reference_is_max_pool2d_with_indices(shape):
    """inputs in {-2..2}: ties everywhere.  Pooled values, the arg-max codes (torch's flat indices converted to ky * 3 + kx) and the
    backward against autograd"""
    B, Hh, W, C = shape
    x = T.int_activations(shape, Hh * 31 + W, "cpu", lim=2).double()
    Ho, Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = T.int_activations((B, Ho, Wo, C), Hh + W, "cpu", lim=8).double()
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    want, ind = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    pooled, code = T.maxpool_idx_reference(x)
    assert torch.equal(pooled, want.detach().permute(0, 2, 3, 1))
    assert torch.equal(code, T.torch_codes(ind, W))
    (want * dy.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(T.maxpool_bwd_reference(code, dy, Hh, W), xn.grad.permute(0, 2, 3, 1))
    if Hh * W > 1:
        n_tied = int(((F.unfold(F.pad(xn.detach(), (1, 1, 1, 1), value=-9.0), 3, stride=2).view(B, C, 9, -1)
                       == pooled.permute(0, 3, 1, 2).reshape(B, C, 1, -1)).sum(dim=2) > 1).sum())
        assert n_tied > 0                                                  # windows with more than one maximum: the first must win


@pytest.mark.parametrize("c", T.WGRAD_CASES, ids=_ids(T.WGRAD_CASES))
def test_conv_wgrad_reference_is_conv2d_autograd(c):
    g = torch.Generator().manual_seed(len(c["tag"]))
    Ho, Wo = T.conv_out(c["H"], c["k"], c["stride"], c["pad"]), T.conv_out(c["W"], c["k"], c["stride"], c["pad"])
    x = torch.randint(-2, 3, (c["B"], c["H"], c["W"], c["Cin"]), generator=g).double()
    dy = torch.randint(-2, 3, (c["B"], Ho, Wo, c["Cout"]), generator=g).double()
    w = torch.zeros(c["Cout"], c["cg"], c["k"], c["k"], dtype=F64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, c["stride"], c["pad"], 1, c["Cin"] // c["cg"])
    assert y.shape == (c["B"], c["Cout"], Ho, Wo)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    ref = T.conv_wgrad_reference(x, dy, c["cg"], c["k"], c["stride"], c["pad"])
    assert torch.equal(ref, w.grad)
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 0     # integers: every fp32 sub-sum is exact


@pytest.mark.parametrize("C,cg", [(32, 1), (64, 2), (128, 4)])
def test_weight_dgrad_reference_gives_the_data_gradient(C, cg):
    """the data gradient of a grouped 3x3 conv equals conv2d(dy, flipped weight, padding=1, groups=32)"""
    g = torch.Generator().manual_seed(C)
    x = torch.randint(-2, 3, (2, C, 5, 6), generator=g).double().requires_grad_()
    w = torch.randint(-2, 3, (C, cg, 3, 3), generator=g).double()
    dy = torch.randint(-2, 3, (2, C, 5, 6), generator=g).double()
    assert C // cg == 32
    (F.conv2d(x, w, None, 1, 1, 1, 32) * dy).sum().backward()
    wf = T.weight_dgrad_reference(w, C, cg)
    assert torch.equal(F.conv2d(dy, wf, None, 1, 1, 1, 32), x.grad)
    # and on w = arange, the operand of the GPU test: the index formula of the kernel, spelled out
    wa = torch.arange(C * cg * 9, dtype=F64).view(C, cg, 3, 3)
    out = T.weight_dgrad_reference(wa, C, cg).flatten()
    i = torch.arange(C * cg * 9)
    t, col, o = i % 9, (i // 9) % cg, i // (9 * cg)
    assert torch.equal(out, ((((o // cg) * cg + col) * cg + o % cg) * 9 + 8 - t).double())


def test_zero_stuff_reference_is_the_stride_2_data_gradient():
    """conv_transpose of a 1x1 stride-2 conv: the zero-stuffed dy is what a stride-1 conv then reads"""
    dy = T.int_activations((2, 3, 5, 8), 1, "cpu").double()
    z = T.zero_stuff_reference(dy)
    x = torch.zeros(2, 8, 6, 10, dtype=F64, requires_grad=True)
    w = torch.eye(8, dtype=F64).view(8, 8, 1, 1)
    (F.conv2d(x, w, None, 2) * dy.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(z, x.grad.permute(0, 2, 3, 1)) and z.shape == (2, 6, 10, 8)


def test_moments_reference_is_batch_norm_statistics():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(512, 9, generator=g, dtype=F64) * 2 + 1
    stats = torch.stack([x.sum(dim=0), (x * x).sum(dim=0)]).float()[None]
    r = T.bn_moments_reference(stats, 512, 1e-5, None)
    assert float((r["mean"] - x.mean(dim=0)).abs().max()) < 1e-6
    assert float((r["rstd"] - 1.0 / torch.sqrt(x.var(dim=0, unbiased=False) + 1e-5)).abs().max()) < 1e-6
    assert float((r["unbiased_rstd"] - 1.0 / torch.sqrt(x.var(dim=0, unbiased=True) + 1e-5)).abs().max()) < 1e-6


@pytest.mark.parametrize("rows", T.MOMENTS_ROWS)
def test_moments_inputs_add_up(rows):
    for C in (4, 100):
        for count in (T.MOMENTS_COUNT, T.MOMENTS_RAGGED_COUNT):
            for neg in (False, True):
                t = T.moments_inputs(rows, C, count, rows + C, "cpu", negative_var=neg)
                r = T.bn_moments_reference(t["stats"], count, 0.25, t["centre"])
                assert torch.equal(r["mean"], t["mean"]) and torch.equal(r["var"], t["var"])
                assert bool((r["raw_var"] < 0).all()) == neg
                assert set(r["rstd"].tolist()) <= {2.0, 1.0, 0.5, 0.25}               # var + 1/4 is a power of four
                assert T.is_f32(r["mean"]) and T.is_f32(r["centre"])
                if not neg:                                                          # an unbiased variance would show
                    moved = r["unbiased_rstd"].float() != r["rstd"].float()
                    assert bool(moved[t["var"] > 0].all())
                r5 = T.bn_moments_reference(t["stats"], count, 1e-5, t["centre"])      # the workload's eps: a real square root
                assert bool(torch.isfinite(r5["rstd"]).all()) and float(r5["rstd"].max()) <= 1.0 / (1e-5 ** 0.5) * 1.001


# ---- the exact cases are exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("c", T.BN_BWD_EXACT, ids=_ids(T.BN_BWD_EXACT))
def test_bn_bwd_exact_cases_are_exact(c, mode):
    epc = T.epc_of(c["dt"])
    p = T.bn_bwd_plan(epc, c["rows"], c["C"])
    t = T.bn_bwd_inputs(c["rows"], c["C"], c["rows"] + c["C"], "cpu")
    assert T.chunk_constants_differ(t)
    for k in ("x", "dy", "out"):
        assert torch.equal(t[k].to(T.BF).float(), t[k])                          # bf16 holds every operand
    r = T.bn_bwd_reference(mode, t["x"], t["out"], t["dy"], t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"])
    bad = T.bn_bwd_exactness(t, r, p)
    assert not bad, (c["tag"], mode, bad)
    pre = t["x"].double() * t["scale"].double() + t["shift"].double()
    assert torch.equal(pre, t["scale"].double() * (t["x"].double() - t["mean"].double() + t["b0"].double()))
    if c["rows"] * c["C"] >= 256:
        assert bool((pre == 0).any()) and bool((pre > 0).any()) and bool((pre < 0).any())      # mode 1: exact zeros to mask
        o = t["out"]
        assert bool(((o == 0) & o.signbit()).any()) and bool(((o == 0) & ~o.signbit()).any()) and bool((o > 0).any())
        if mode:
            assert bool((r["g"] != t["dy"].double()).any())                        # the mask masks
    if c["dt"] == "bf16" and c["rows"] >= 64:
        assert not torch.equal(r["dx"].float().to(T.BF).double(), r["dx"])           # the bf16 rounding of dx is a real one


def test_an_inexact_case_fails_on_the_host():
    """what the check above is worth: three rows (1 / 3 is rounded) and operands too large for 24 bits are both reported"""
    t = T.bn_bwd_inputs(3, 8, 1, "cpu")
    r = T.bn_bwd_reference(0, t["x"], t["out"], t["dy"], t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"])
    bad = T.bn_bwd_exactness(t, r, T.bn_bwd_plan(8, 3, 8))
    assert any("power of two" in b for b in bad) and any("not representable" in b for b in bad), bad
    t = T.bn_bwd_inputs(4096, 8, 1, "cpu", lim=4000)
    r = T.bn_bwd_reference(0, t["x"], t["out"], t["dy"], t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"])
    assert T.bn_bwd_exactness(t, r, T.bn_bwd_plan(8, 4096, 8))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_bwd_ragged_sums_stay_exact(dt):
    """rows no power of two: dbeta, dgamma (and g) are still exact -- only 1 / n and what follows it are rounded"""
    for C in T.bn_bwd_ragged_channels(dt)[:3]:
        for rows in T.BN_BWD_RAGGED_ROWS:
            p = T.bn_bwd_plan(T.epc_of(dt), rows, C)
            t = T.bn_bwd_inputs(rows, C, rows + C, "cpu")
            for mode in (0, 1, 2):
                r = T.bn_bwd_reference(mode, t["x"], t["out"], t["dy"], t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"])
                bad = [b for b in T.bn_bwd_exactness(t, r, p) if "dbeta is" in b or "dgamma is" in b or "2^24" in b]
                assert not bad, (dt, C, rows, mode, bad)


# ---- regimes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.BN_BWD_EXACT, ids=_ids(T.BN_BWD_EXACT))
def test_bn_bwd_cases_are_in_their_regime(c):
    epc = T.epc_of(c["dt"])
    assert T.bn_bwd_supported(c["C"], epc)
    p = T.bn_bwd_plan(epc, c["rows"], c["C"])
    for k in T.BN_BWD_CLAIMS:
        if k in c:
            assert p[k] == c[k], (c["tag"], k, p)
    assert (p["agrid"] * 256) % p["cc"] == 0


def test_bn_bwd_table_reaches_every_regime():
    plans = [T.bn_bwd_plan(T.epc_of(c["dt"]), c["rows"], c["C"]) for c in T.BN_BWD_EXACT]
    assert any(p["idle_lanes"] > 0 for p in plans) and any(p["partial_unroll"] and p["rows_per_lane"] in (2, 3) for p in plans)
    assert any(p["trips"] == 1 and p["rows_per_lane"] == 1 for p in plans) and any(p["trips"] > 1 for p in plans)
    assert any(p["ny"] == 2 for p in plans) and any(p["capped"] and p["finalize_reads"] == 8 for p in plans)
    assert any(p["cc"] == 1 for p in plans) and {p["RL"] for p in plans} >= {1, 4, 32, 256}
    ragged = [T.bn_bwd_plan(T.epc_of(dt), rows, C) for dt in ("f32", "bf16") for C in T.bn_bwd_ragged_channels(dt)
              for rows in T.BN_BWD_RAGGED_ROWS]
    assert any(p["g"] > 1 and p["partial_unroll"] for p in ragged) and any(p["atrips"] > 1 for p in ragged)
    assert not T.bn_bwd_supported(24, 8) and not T.bn_bwd_supported(12, 4) and T.bn_bwd_supported(8, 8)


def test_bn_bwd_rows_is_the_library_s():
    """the restatement against cvcl_bn_bwd_partial_rows (a host function: no device needed)"""
    lib = H.lib()
    for dt, cd in (("f32", H.F32), ("bf16", H.BF16)):
        epc = T.epc_of(dt)
        for C in (epc, 2 * epc, 64, 256, 1024, 2048, 4096, 8192):
            for rows in (1, 2, 3, 7, 8, 9, 63, 64, 65, 98, 1000, 1024, 1100, 4096, 4097, 8192, 65536, 802816):
                assert lib.cvcl_bn_bwd_partial_rows(cd, rows, C) == T.bn_bwd_rows(epc, rows, C), (dt, rows, C)
    for c in T.BN_BWD_EXACT:
        cd = H.BF16 if c["dt"] == "bf16" else H.F32
        assert lib.cvcl_bn_bwd_partial_rows(cd, c["rows"], c["C"]) == T.bn_bwd_plan(T.epc_of(c["dt"]), c["rows"], c["C"])["g"]


def test_bn_apply_grids():
    for epc in (4, 8):
        for cc in T.BN_APPLY_CC:
            assert T.bn_apply_supported(cc * epc, epc)
            for rows in T.AFFINE_ROWS:
                p = T.bn_apply_plan(rows, cc * epc, epc)
                assert p["fixed_chunk"] and p["grid"] % (3 if cc == 768 else 1) == 0, p
        assert not T.bn_apply_supported(3 * epc, epc) and not T.bn_apply_supported(epc + 1, epc)
        p = T.bn_apply_plan(98, 768 * epc, epc)                                    # 74 workgroups' worth of chunks -> 75
        assert (p["capped"], p["grid"], p["rounded"]) == (74, 75, True)
    rows, C = T.BN_APPLY_PAST_CAP
    p = T.bn_apply_plan(rows, C, 8)
    assert p["total"] == 16777728 and p["capped"] == 16384 and p["grid"] == 16386 and p["trips"] == 4 and p["fixed_chunk"], p
    assert T.chunk_grid(10, 1, 4) == 1 and T.chunk_grid(5000, 5, 4) == 5 and T.chunk_grid(1 << 30, 512, 4) == 16384


def test_flat_grids_pass_their_cap():
    cap = T.GRID_CAP * 256
    B, Hh, W, C = T.MAXPOOL_FWD_PAST_CAP
    units = B * ((Hh - 1) // 2 + 1) * ((W - 1) // 2 + 1) * C // 4
    assert cap < units < cap * 1.05 and T.trips(units, T.flat_plan(units)) == 2
    B, Hh, W, C = T.MAXPOOL_BWD_PAST_CAP
    assert cap < B * Hh * W * C // 4 < cap * 1.05
    B, HW, C = T.AVGPOOL_BWD_PAST_CAP
    assert cap < B * HW * C < cap * 1.05 and T.trips(B * HW * C, T.flat_plan(B * HW * C)) == 2
    B, Ho, Wo, C = T.ZERO_STUFF_PAST_CAP
    assert cap < B * 4 * Ho * Wo * C // 4 < cap * 1.05
    n = T.FLAT_PAST_CAP_CHUNKS * 4
    p = T.flat_plan(n)                                                    # cvcl_add / cvcl_relu_mask size their grid by elements
    assert p["grid"] == T.GRID_CAP and T.trips(n // 4, p) == 2
    for chunks in T.FLAT_CHUNKS:
        assert T.trips(chunks, T.flat_plan(chunks * 4)) == 1
    for shape in T.MAXPOOL_IDX_SHAPES:
        assert shape[3] == 8
    assert {(s[1] % 2, s[2] % 2) for s in T.MAXPOOL_IDX_SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_finite_bits_are_finite_and_varied():
    for dt, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        b = T.finite_bits((64, 512), dt, 3, "cpu")
        v = b.view(tdt)
        assert bool(torch.isfinite(v.float()).all()) and bool((v.float() < 0).any()) and len(torch.unique(b)) > 10000
