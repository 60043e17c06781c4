"""GPU: every schedule of cvcl_gconv3x3 through the C ABI, exactly, against float64 (tests/gconv_cases.py).

The operands are small integers and halves on which every fp32 product and partial sum is exact in any order, so the bf16 kernel
(gconv_mfma_kernel<WIDE, NPF, NMT>, all 16 instantiations) must return the bf16 rounding of the float64 result and the fp32 kernels
(gconv_tiled_f32_kernel<CG>, gconv_direct_f32_kernel) the float64 result itself, bit for bit but for the sign of a zero -- at several
work items per workgroup, in the XCD-major item order, with partial last bands, odd maps under stride 2 and one-pixel maps.  Every
case first asserts, from cvcl_gconv3x3_stats_rows and the plan restatements, that it runs in the regime it was chosen for.  A
failure names the first wrong (b, oy, ox, c) and its band, m-tile and work item.

Statistics: a workgroup's partial is an fp32 sum of multiples of 0.5 (squares: of 0.25); where it stays below 2^24 such units it is
exact, and the float64 column sums of the partial rows must equal the float64 sums of the expected output.  That holds for every sum
and for every channel's sum of squares whose total is below 2^24 (asserted), and for most above; for the remaining channels the
existing 2e-5 of check_stats applies (each case prints how many channels were checked which way)."""
import zlib

import pytest
import torch

from multimodal import _hip as H

import gconv_cases as T
from conftest import maxrel
from test_resnext_gpu import check_stats

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
CANARY16 = 0x7B7B                                     # bit pattern of the bf16 output's canary tail (a finite value no case produces)
_CACHE = {}


def _ids(cases):
    return [c["tag"] for c in cases]


def _pack(cd, w):
    C, cg = w.shape[0], w.shape[1]
    nb = H.lib().cvcl_packed_weight_bytes(cd, H.PACK_GCONV3, C, cg, 3)
    buf = torch.empty(nb, dtype=torch.uint8, device=w.device)
    H.check(H.lib().cvcl_pack_conv_weight(cd, H.PACK_GCONV3, H.ptr(w.contiguous()), H.ptr(buf), C, cg, 3, H.stream_ptr()), "pack")
    return buf


def _operands(c, dev, prologue, centre):
    """operands and expected bf16 output of a bf16 case, computed once and never written to"""
    key = (c["tag"], prologue, centre)
    if key not in _CACHE:
        t = T.gconv_inputs(c, zlib.crc32(repr(key).encode()), dev, prologue=prologue, centre=centre)
        ref = T.gconv_reference(t["x"], t["scale"], t["shift"], t["w"], t["centre"], c["stride"], T.GROUPS)
        assert float(ref.abs().max()) <= t["bound"]
        t["exp"] = ref.float().to(BF)                                          # exact in fp32, then the kernel's own final rounding
        t["x16"] = t["x"].to(BF)
        t["wp"] = _pack(H.BF16, t["w"])
        torch.cuda.synchronize()
        _CACHE[key] = t
    return _CACHE[key]


def _launch(cd, c, x, t, wp, y, st, rows):
    return H.lib().cvcl_gconv3x3(cd, H.ptr(x), H.ptr(t["scale"]), H.ptr(t["shift"]), H.ptr(wp), H.ptr(y), H.ptr(st), rows,
                                 H.ptr(t["centre"]), c["B"], c["H"], c["W"], c["C"], T.GROUPS, c["stride"],
                                 H.stream_ptr())


def _bf16_buffers(c, dev, rows):
    """y with a canary tail of one output row behind it, statistics rows with one canary row behind them"""
    Ho, Wo = T.out_hw(c["H"], c["W"], c["stride"])
    n, tail = c["B"] * Ho * Wo * c["C"], Wo * c["C"]
    raw = torch.full((n + tail,), CANARY16, dtype=torch.int16, device=dev)
    y = raw[:n].view(BF).view(c["B"], Ho, Wo, c["C"])
    st = torch.full((rows + 1, 2, c["C"]), float("nan"), device=dev)
    return raw, y, st, n


def _where_wrong(y, exp, TH, bands, Wo, grid=None):
    bad = (y != exp) | y.isnan()
    n_bad = int(bad.sum())
    if not n_bad:
        return ""
    b, oy, ox, ch = bad.nonzero()[0].tolist()
    band, q = oy // TH, (oy % TH) * Wo + ox
    msg = (f"{n_bad} of {y.numel()} wrong; first at (b, oy, ox, c) = ({b}, {oy}, {ox}, {ch}): got {float(y[b, oy, ox, ch])}, want "
           f"{float(exp[b, oy, ox, ch])}; band {band} of {bands} (TH {TH}), row {oy % TH} of the band, band pixel {q}, m-tile {q // 16}, "
           f"work item {b * bands + band}")
    if grid:
        msg += f", trip {(b * bands + band) // grid} of a grid of {grid}"
    bad_b = bad.flatten(1).any(1).nonzero().flatten().tolist()
    return msg + f"; images with wrong values: {bad_b[:8]}{'...' if len(bad_b) > 8 else ''}"


def _check_regime(c, p, rows):
    assert p["supported"] and rows == p["grid_x"], (rows, p)
    if c.get("inst") is not None:
        assert p["inst"] == c["inst"], p
    if c.get("multi"):
        assert rows < c["B"] * p["bands"], (rows, p)
    if c.get("xcd"):
        assert rows % 8 == 0, rows
    if "xcd" in c and not c["xcd"]:
        assert rows % 8 != 0 and rows == c["B"] * p["bands"], rows
    if c.get("partial"):
        assert p["partial"], p


def _wg_partials(v, p, grid):
    """v [B, Ho, Wo, C] float64, non-negative -> [C]: the largest sum any workgroup accumulates.  Work item (b, band) = b * bands +
    band goes to the workgroup that holds item % grid (a grid-stride loop: true in the plain and in the XCD-major order alike)."""
    B, Ho, Wo, C = v.shape
    TH, bands = p["TH"], p["bands"]
    per_item = torch.nn.functional.pad(v, (0, 0, 0, 0, 0, bands * TH - Ho)).view(B * bands, TH * Wo, C).sum(dim=1)
    trips = -(-per_item.shape[0] // grid)
    per_wg = torch.nn.functional.pad(per_item, (0, 0, 0, trips * grid - per_item.shape[0])).view(trips, grid, C).sum(dim=0)
    return per_wg.max(dim=0).values


def _check_sums(tag, s, exp, p, grid):
    """s [2, C] float64 column sums the kernel reported; exp the expected bf16 output.  A workgroup adds its values in fp32 and hands
    on one partial per channel; the partials are added in float64 (here) or as int64 fixed point (accumulators).  The values are
    multiples of 0.5, their squares of 0.25 (of 1 in a channel without halves): where a workgroup's sum of magnitudes stays below
    2^24 such units, every fp32 sub-sum in any order is exact and the reported total must EQUAL the float64 one."""
    C = exp.shape[-1]
    e4 = exp.double()
    e = e4.reshape(-1, C)
    assert float(_wg_partials(e4.abs(), p, grid).max()) * 2 < 2 ** 24
    assert torch.equal(s[0], e.sum(dim=0)), (tag, float((s[0] - e.sum(dim=0)).abs().max()))
    sq = (e * e).sum(dim=0)
    quantum = torch.where(((e * 2) % 2 != 0).any(dim=0), 0.25, 1.0).to(F64)
    exact = _wg_partials(e4 * e4, p, grid) / quantum < 2 ** 24
    assert bool(exact[sq < 2 ** 24].all())                 # (no less than every channel whose total is below 2^24)
    print(f"{tag}: sums of squares exact on {int(exact.sum())} of {C} channels ({int((sq < 2 ** 24).sum())} have a total below 2^24), "
          f"at 2e-5 on {int((~exact).sum())} (largest total {float(sq.max()):.0f})")
    assert torch.equal(s[1][exact], sq[exact]), (tag, float((s[1] - sq)[exact].abs().max()))
    assert maxrel(s[1], sq) < 2e-5


def _run_bf16(c, dev, prologue=True, centre=True, repeat=True):
    lib = H.lib()
    p = T.bf16_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])
    rows = lib.cvcl_gconv3x3_stats_rows(H.BF16, c["B"], c["H"], c["W"], c["C"], c["stride"])
    _check_regime(c, p, rows)
    Ho, Wo = T.out_hw(c["H"], c["W"], c["stride"])
    t = _operands(c, dev, prologue, centre)
    raw, y, st, n = _bf16_buffers(c, dev, rows)
    H.check(_launch(H.BF16, c, t["x16"], t, t["wp"], y, st, rows), "gconv")
    torch.cuda.synchronize()
    wrong = _where_wrong(y, t["exp"], p["TH"], p["bands"], Wo, rows)
    assert not wrong, f"{c['tag']} {p['inst']}: {wrong}"
    assert y.dtype == t["exp"].dtype and y.shape == t["exp"].shape and torch.equal(y, t["exp"])
    assert bool((raw[n:] == CANARY16).all()), "wrote behind y"
    assert bool(st[rows].isnan().all()), "wrote behind the statistics rows"
    assert bool(torch.isfinite(st[:rows]).all())
    _check_sums(c["tag"], st[:rows].double().sum(dim=0), t["exp"], p, rows)
    if repeat:                                             # a second launch on the same buffers: the same bits
        y1, st1 = raw.clone(), st.clone()
        H.check(_launch(H.BF16, c, t["x16"], t, t["wp"], y, st, rows), "gconv again")
        torch.cuda.synchronize()
        assert torch.equal(raw, y1) and torch.equal(st.view(torch.int32), st1.view(torch.int32))
    return raw, y, st


@pytest.mark.parametrize("c", T.TRUNK_CASES, ids=_ids(T.TRUNK_CASES))
def test_bf16_trunk_geometries_several_items_per_workgroup(dev, c):
    """the work-item loop's later trips (register prefetch of the next item, the barrier between one item's LDS readers and the next
    item's staging, statistics across items), the XCD-major item order and the plain one, the partial band of layer3.0"""
    _run_bf16(c, dev)


@pytest.mark.parametrize("c", T.EDGE_CASES, ids=_ids(T.EDGE_CASES))
def test_bf16_instantiations_and_edge_geometry(dev, c):
    """the instantiations the trunk's shapes do not reach, and odd, non-square, one-row, one-pixel and widest-row maps, narrow and wide"""
    _run_bf16(c, dev)


@pytest.mark.parametrize("tag", T.VARIATION_TAGS)
@pytest.mark.parametrize("prologue,centre", [(False, True), (True, False), (False, False)], ids=["no_prologue", "no_centre", "plain"])
def test_bf16_without_prologue_or_centre(dev, tag, prologue, centre):
    """a_scale = a_shift = NULL is the data-gradient use: no activation, negative inputs pass unclipped; centre = NULL subtracts nothing"""
    c = T.by_tag(tag)
    t = _operands(c, dev, prologue, centre)
    if not prologue:
        assert t["scale"] is None and t["shift"] is None and float(t["x"].min()) < 0
        clipped = T.gconv_reference(torch.relu(t["x"]), None, None, t["w"], t["centre"], c["stride"], T.GROUPS).float().to(BF)
        assert not torch.equal(clipped, t["exp"])          # (the case can tell a ReLU that should not be there)
    _run_bf16(c, dev, prologue, centre, repeat=False)


def test_bf16_without_statistics_is_the_same_output(dev):
    c = T.by_tag("l3_28_s2_B25")
    t = _operands(c, dev, True, True)
    rows = H.lib().cvcl_gconv3x3_stats_rows(H.BF16, c["B"], c["H"], c["W"], c["C"], c["stride"])
    raw, y, _st, n = _bf16_buffers(c, dev, rows)
    H.check(_launch(H.BF16, c, t["x16"], t, t["wp"], y, None, 0), "gconv, stats = NULL")
    torch.cuda.synchronize()
    assert torch.equal(y, t["exp"]) and bool((raw[n:] == CANARY16).all())
    raw2, _y2, _st2 = _run_bf16(c, dev, repeat=False)
    assert torch.equal(raw, raw2)                         # bit for bit what the launch with statistics stores


@pytest.mark.parametrize("tag", T.ACCUMULATE_TAGS)
def test_bf16_statistics_accumulators(dev, tag):
    """stats_rows == CVCL_STATS_ACCUMULATE: int64 [8][2][C] fixed point with 24 fractional bits, one row per XCD; a half-integer
    partial converts exactly, integer addition commutes: the 8 rows add up to the exact sums."""
    c = T.by_tag(tag)
    p = T.bf16_plan(c["B"], c["H"], c["W"], c["C"], c["stride"])
    assert p["grid_x"] < p["items"]
    t = _operands(c, dev, True, True)
    Ho, Wo = T.out_hw(c["H"], c["W"], c["stride"])
    raw, y, _st, n = _bf16_buffers(c, dev, 1)
    acc = torch.zeros(8 + 1, 2, c["C"], dtype=torch.int64, device=dev)
    acc[8] = -12345
    for launch in (1, 2):                                 # the accumulators ADD: a second launch doubles them
        H.check(_launch(H.BF16, c, t["x16"], t, t["wp"], y, acc, H.STATS_ACCUMULATE), "gconv, accumulators")
        torch.cuda.synchronize()
        wrong = _where_wrong(y, t["exp"], p["TH"], p["bands"], Wo, p["grid_x"])
        assert not wrong, wrong
        assert bool((raw[n:] == CANARY16).all()) and bool((acc[8] == -12345).all())
        tot = acc[:8].sum(dim=0)
        assert bool((tot % launch == 0).all())
        _check_sums(f"{tag} (accumulators, launch {launch})", (tot // launch).double() / 2 ** 24, t["exp"], p, p["grid_x"])


@pytest.mark.parametrize("r", T.REFUSALS, ids=_ids(T.REFUSALS))
def test_bf16_refusals_launch_nothing(dev, r):
    lib = H.lib()
    Ho, Wo = T.out_hw(r["H"], r["W"], r["stride"])
    C = r["C"]
    x = torch.ones(r["B"], r["H"], r["W"], C, dtype=BF, device=dev)
    wp = torch.zeros(C * 32 * 9 * 4, dtype=torch.uint8, device=dev)               # (never read: at least any packed size)
    sc, sh, cen = torch.ones(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rows = max(lib.cvcl_gconv3x3_stats_rows(H.BF16, r["B"], r["H"], r["W"], C, r["stride"]), 2)
    y = torch.full((r["B"], Ho, Wo, C), CANARY16, dtype=torch.int16, device=dev)
    st = torch.full((rows, 2, C), float("nan"), device=dev)
    rc = lib.cvcl_gconv3x3(H.BF16, H.ptr(x), H.ptr(sc), H.ptr(sh), H.ptr(wp), H.ptr(y), H.ptr(st), rows - r.get("rows_short", 0),
                           H.ptr(cen), r["B"], r["H"], r["W"], C, T.GROUPS, r["stride"], H.stream_ptr())
    assert rc == H.EINVAL
    msg = lib.cvcl_last_error().decode()
    assert r["msg"] in msg and "cvcl_gconv3x3" in msg, msg
    torch.cuda.synchronize()
    assert bool((y == CANARY16).all()) and bool(st.isnan().all())


# ---- fp32 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.F32_CASES, ids=_ids(T.F32_CASES))
def test_f32_exact(dev, c):
    """dtype = CVCL_F32: the float64 result cast to fp32, bit for bit.  The tiled kernel at more (image, band) items than workgroups
    for each channels-per-group, a partial last band, pixel blocks with idle lanes, odd and one-pixel maps; and an x pointer one
    float off 16-byte alignment, which takes the direct kernel on a trunk shape."""
    lib = H.lib()
    p = T.f32_plan(c["B"], c["H"], c["W"], c["C"], c["stride"], aligned=not c.get("misaligned"))
    assert p["tiled"] == (not c.get("misaligned"))
    if c.get("second_trip"):
        assert p["items"] > p["gx"], p
    if c.get("partial"):
        assert p["partial"], p
    Ho, Wo = T.out_hw(c["H"], c["W"], c["stride"])
    t = T.gconv_inputs(c, 77 + c["C"] + c["H"], dev)
    exp = T.gconv_reference(t["x"], t["scale"], t["shift"], t["w"], t["centre"], c["stride"], T.GROUPS).float()
    x = t["x"]
    if c.get("misaligned"):
        xb = torch.empty(x.numel() + 4, device=dev)
        xb[1:1 + x.numel()] = x.flatten()
        x = xb[1:1 + x.numel()]
        assert x.data_ptr() % 16 == 4
    wp = _pack(H.F32, t["w"])
    rows = lib.cvcl_gconv3x3_stats_rows(H.F32, c["B"], c["H"], c["W"], c["C"], c["stride"])
    n, tail = exp.numel(), Wo * c["C"]
    raw = torch.full((n + tail,), float("nan"), device=dev)
    y = raw[:n].view(exp.shape)
    st = torch.full((rows + 1, 2, c["C"]), float("nan"), device=dev)
    H.check(_launch(H.F32, c, x, t, wp, y, st, rows), "gconv f32")
    torch.cuda.synchronize()
    wrong = _where_wrong(y, exp, p["TH"], p["bands"], Wo, p["gx"] if p["tiled"] else None)
    assert not wrong, f"{c['tag']} {'tiled' if p['tiled'] else 'direct'}: {wrong}"
    assert torch.equal(y, exp)
    assert bool(raw[n:].isnan().all()) and bool(st[rows].isnan().all())
    check_stats(st, rows, y)
