"""GPU: the ResNeXt forward kernels around the grouped convolution, one by one through the C ABI, exactly, against float64
(tests/stem_cases.py): the four stem kernels, bn_finalize, bn_eval_affine, col_stats, bn_relu_maxpool, bn_add_relu, bn_relu_apply,
avgpool and the stem weight packer.

The operands are small integers, halves and eighths and power-of-two scales, on which every fp32 product, sum, fmaf and maximum is
exact in any order: an fp32 kernel must return the float64 result and a bf16 kernel its bf16 rounding, bit for bit but for the sign
of a zero.  Every case first asserts, from the launcher restatements (and from cvcl_stem_conv_stats_rows / cvcl_col_stats_rows
where the ABI shows the grid), that it runs in the regime it was chosen for: which fp32 stem kernel, a shrunk or partial band, a
second grid-stride trip, the XCD-major item order, a grid rounded for the fixed channel chunk.  Outputs and statistics rows have a
canary row behind them; statistics rows start as NaN and exactly ``stats_rows`` of them must have been written.  A failure names
the first wrong element and the band, m-tile, work item, workgroup and trip that computed it.

The only comparisons that are not equalities are the random cases of bn_finalize / bn_eval_affine: per-channel bounds derived in
test_bn_finalize_random_within_the_derived_bounds from the kernel's operation sequence."""
import zlib

import pytest
import torch

from multimodal import _hip as H

import stem_cases as T

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
CANARY16 = 0x7B7B                                     # bit pattern of a bf16 canary (a finite value no case produces)
U = 2.0 ** -24                                        # unit roundoff of fp32
_CACHE = {}


def _ids(cases):
    return [c["tag"] for c in cases]


def _dt(dt):
    return (H.BF16, BF, 8) if dt == "bf16" else (H.F32, F32, 4)


def _claims(c, p, keys):
    for k in keys:
        if k in c:
            assert p[k] == c[k], (c["tag"], k, p)


def _out(shape, tdt, dev, tail):
    """an output tensor of ``shape`` with ``tail`` canary elements behind it -> (whole buffer, view, n)"""
    n = 1
    for s in shape:
        n *= s
    if tdt == BF:
        raw = torch.full((n + tail,), CANARY16, dtype=torch.int16, device=dev)
        return raw, raw[:n].view(BF).view(shape), n
    raw = torch.full((n + tail,), float("nan"), dtype=tdt, device=dev)
    return raw, raw[:n].view(shape), n


def _tail_intact(raw, n):
    return bool((raw[n:] == CANARY16).all()) if raw.dtype == torch.int16 else bool(raw[n:].isnan().all())


def _expected(ref64, tdt):
    """the float64 result as the kernel must store it: exact in fp32 (asserted), then the bf16 rounding where it stores bf16"""
    e = ref64.float()
    assert torch.equal(e.double(), ref64)
    return e.to(BF) if tdt == BF else e


def _first_wrong(y, exp):
    bad = (y != exp) | y.isnan()
    n_bad = int(bad.sum())
    if not n_bad:
        return None
    idx = bad.nonzero()[0].tolist()
    return n_bad, idx, f"{n_bad} of {y.numel()} wrong; first at {tuple(idx)}: got {float(y[tuple(idx)])}, want {float(exp[tuple(idx)])}"


def _where_wrong(y, exp, p, what="(b, oy, ox, c)"):
    """y, exp [B, rows, cols, C] of a kernel that walks (image, band of p['TH'] rows) work items on a grid of p['grid']"""
    w = _first_wrong(y, exp)
    if w is None:
        return ""
    _n, (b, oy, ox, ch), msg = w
    band, item = oy // p["TH"], b * p["bands"] + oy // p["TH"]
    msg = (f"{what} {msg}; band {band} of {p['bands']} (TH {p['TH']}), row {oy % p['TH']} of the band, m-tile {ox // 16} of its row "
           f"(lane pixel {ox % 16}), work item {item}, workgroup bx {T.item_workgroup(item, p['grid'])}, trip {item // p['grid']} of a "
           f"grid of {p['grid']}")
    bad = (y != exp) | y.isnan()
    return msg + f"; wrong channels: {bad.flatten(0, 2).any(0).nonzero().flatten().tolist()[:40]}"


def _where_flat(y, exp, chunk, stride):
    """y, exp [rows, C] of a kernel whose thread i0 takes the ``chunk``-element pieces i0, i0 + stride, ..."""
    w = _first_wrong(y, exp)
    if w is None:
        return ""
    _n, (r, ch), msg = w
    i = (r * y.shape[1] + ch) // chunk
    return f"{msg}; chunk {i} (channel chunk {i % (y.shape[1] // chunk)}), thread {i % stride}, trip {i // stride} at a stride of {stride}"


# ---- the stem's operands -----------------------------------------------------------------------------------------------------------
def _pack_stem(cd, w, dev):
    """cvcl_pack_conv_weight(STEM7) into a canary-filled buffer: cvcl_packed_weight_bytes bytes are written, and no more"""
    nb = H.lib().cvcl_packed_weight_bytes(cd, H.PACK_STEM7, 64, 3, 7)
    assert nb == (4 * 6 * 16 * 32 * 2 if cd == H.BF16 else 64 * 3 * 49 * 4)
    buf = torch.full((nb + 256,), 0xA5, dtype=torch.uint8, device=dev)
    wd = w.to(dev).contiguous()
    H.check(H.lib().cvcl_pack_conv_weight(cd, H.PACK_STEM7, H.ptr(wd), H.ptr(buf), 64, 3, 7, H.stream_ptr()), "pack")
    torch.cuda.synchronize()
    assert bool((buf[nb:] == 0xA5).all()), "the packer wrote behind cvcl_packed_weight_bytes"
    words = buf[:nb].view(torch.int16)
    assert not bool((words == torch.tensor(0xA5A5 - 65536, dtype=torch.int16)).any()), "the packer left part of its output unwritten"
    return buf[:nb]


def _stem_ops(c, dev, centre):
    """operands and the float64 reference of a stem case, computed once and never written to"""
    key = (c["B"], c["H"], c["W"], centre)
    if key not in _CACHE:
        x, w, cen = T.stem_inputs(c["B"], c["H"], c["W"], zlib.crc32(repr(key).encode()), centre=centre)
        t = dict(x=x.to(dev), w=w.to(dev), cen=None if cen is None else cen.to(dev))
        t["ref"] = T.stem_reference(t["x"], t["w"], t["cen"])
        assert float(t["ref"].abs().max()) * 2 < 2 ** 24 and torch.equal(t["ref"].float().double(), t["ref"])
        t["wp16"], t["wp32"] = _pack_stem(H.BF16, w, dev), _pack_stem(H.F32, w, dev)
        _CACHE[key] = t
    return _CACHE[key]


# ---- cvcl_stem_conv7x7, bf16 ------------------------------------------------------------------------------------------------------
def _check_stem_sums(tag, st, exp, p):
    """st [rows, 2, 64] partial rows, exp the expected bf16 output.  A workgroup adds its rounded outputs and their squares in fp32
    and hands on one partial per channel.  The outputs are multiples of 0.5, their squares of 0.25 (of 1 in a channel without
    halves): the largest partial any workgroup forms stays below 2^24 such units in EVERY channel (asserted), so every fp32
    sub-sum in any order is exact and the float64 column sums of the partial rows must EQUAL those of the expected output."""
    s_units, q_units = T.stem_stats_bound(exp, p)
    assert s_units < 2 ** 24 and q_units < 2 ** 24, (tag, s_units, q_units)
    e = exp.double().reshape(-1, 64)
    s = st.double().sum(dim=0)
    bad = ((s[0] != e.sum(dim=0)) | (s[1] != (e * e).sum(dim=0))).nonzero().flatten().tolist()
    assert not bad, (f"{tag}: statistics wrong in channels {bad[:16]}: sum off by {float((s[0] - e.sum(dim=0)).abs().max())}, "
                     f"sum of squares by {float((s[1] - (e * e).sum(dim=0)).abs().max())}")


def _run_bf16_stem(c, dev, centre, store=True):
    lib = H.lib()
    B, Hh, W = c["B"], c["H"], c["W"]
    p = T.bf16_stem_plan(B, Hh, W)
    rows = lib.cvcl_stem_conv_stats_rows(H.BF16, B, Hh, W)
    assert p["supported"] and rows == p["grid"], (rows, p)
    _claims(c, p, ("bands", "items", "grid", "xcd", "trips", "mtiles", "partial_band", "partial_tile"))
    t = _stem_ops(c, dev, centre)
    exp = t["ref"].float().to(BF)
    assert float(t["ref"].abs().max()) > 256 and not torch.equal(exp.double(), t["ref"])      # the bf16 rounding is a real one
    raw, y, n = _out((B, p["Ho"], p["Wo"], 64), BF, dev, p["Wo"] * 64)
    st = torch.full((rows + 1, 2, 64), float("nan"), device=dev)
    H.check(lib.cvcl_stem_conv7x7(H.BF16, H.ptr(t["x"]), H.ptr(t["wp16"]), H.ptr(y) if store else None, H.ptr(st), rows,
                                  H.ptr(t["cen"]), B, Hh, W, H.stream_ptr()), "stem bf16")
    torch.cuda.synchronize()
    if store:
        wrong = _where_wrong(y, exp, p)
        assert not wrong, f"{c['tag']} centre={centre}: {wrong}"
        assert y.dtype == exp.dtype and torch.equal(y, exp)
    else:
        assert bool((raw == CANARY16).all()), "a statistics-only launch wrote an output"
    assert _tail_intact(raw, n), "wrote behind y"
    assert bool(st[rows].isnan().all()), "wrote behind the statistics rows"
    assert bool(torch.isfinite(st[:rows]).all()), "a statistics row was left unwritten"
    _check_stem_sums(c["tag"], st[:rows], exp, p)
    return y, st


@pytest.mark.parametrize("centre", [True, False], ids=["centred", "plain"])
@pytest.mark.parametrize("c", T.BF16_STEM_CASES, ids=_ids(T.BF16_STEM_CASES))
def test_stem_bf16_exact(dev, c, centre):
    """stem_mfma_kernel: one band, a partial last band with a partial last m-tile, H != W, the widest row, fewer tiles than waves,
    a second trip of the item loop in the XCD-major order, and the plain order"""
    _run_bf16_stem(c, dev, centre)


def test_stem_bf16_statistics_only_is_the_storing_run(dev):
    """y = NULL: the same statistics rows bit for bit, and nothing stored anywhere"""
    (c,) = [c for c in T.BF16_STEM_CASES if c["tag"] == "second_trip_65x64x64"]
    _y, st_a = _run_bf16_stem(c, dev, True)
    _y, st_b = _run_bf16_stem(c, dev, True, store=False)
    assert torch.equal(st_a[:-1].view(torch.int32), st_b[:-1].view(torch.int32))


@pytest.mark.parametrize("r", T.BF16_STEM_REFUSALS, ids=_ids(T.BF16_STEM_REFUSALS))
def test_stem_bf16_refusals_launch_nothing(dev, r):
    B, Hh, W = r["B"], r["H"], r["W"]
    assert not T.bf16_stem_supported(Hh, W)
    x = torch.ones(B, 3, Hh, W, device=dev)
    wp = torch.zeros(4 * 6 * 512 * 2, dtype=torch.uint8, device=dev)
    rows = max(H.lib().cvcl_stem_conv_stats_rows(H.BF16, B, Hh, W), 1)
    y = torch.full((B, (Hh + 1) // 2, (W + 1) // 2, 64), CANARY16, dtype=torch.int16, device=dev)
    st = torch.full((rows, 2, 64), float("nan"), device=dev)
    rc = H.lib().cvcl_stem_conv7x7(H.BF16, H.ptr(x), H.ptr(wp), H.ptr(y), H.ptr(st), rows, None, B, Hh, W, H.stream_ptr())
    assert rc == H.EINVAL and "cvcl_stem_conv7x7" in H.lib().cvcl_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == CANARY16).all()) and bool(st.isnan().all())


# ---- cvcl_stem_conv7x7, fp32 ------------------------------------------------------------------------------------------------------
def _check_col_stats_rows(tag, st, y2d, g):
    """st [g, 2, C] partial rows of col_stats_kernel over y2d [rows, C] (any float dtype): block k adds rows 4 k + slice + 4 g j
    in fp32.  Where the largest partial stays below 2^24 units (asserted) each partial row is exact: checked row by row."""
    s_units, q_units = T.col_stats_bound(y2d, g)
    assert s_units < 2 ** 24 and q_units < 2 ** 24, (tag, s_units, q_units)
    e = y2d.double()
    blk = T.col_stats_block(e.shape[0], g).to(e.device)
    z = torch.zeros(g, e.shape[1], dtype=F64, device=e.device)
    want = torch.stack([z.index_add(0, blk, e), z.index_add(0, blk, e * e)], dim=1)
    bad = (st.double() != want).nonzero()
    assert not len(bad), f"{tag}: {len(bad)} partial sums wrong; first at (partial row, sum | squares, channel) = {bad[0].tolist()}"


@pytest.mark.parametrize("centre", [True, False], ids=["centred", "plain"])
@pytest.mark.parametrize("c", T.F32_STEM_CASES, ids=_ids(T.F32_STEM_CASES))
def test_stem_f32_exact(dev, c, centre):
    """dtype = CVCL_F32: the float64 result itself.  stem_tiled_f32_kernel at TH = 8, with a partial band, with a band shrunk to 7
    rows and to 1 row, and past its 1024 workgroups; stem_direct_f32_kernel at the first widths whose one-row band does not fit.
    The ABI does not show which kernel ran: the launcher's restatement (f32_stem_plan) is the check of the regime."""
    lib = H.lib()
    B, Hh, W = c["B"], c["H"], c["W"]
    p = T.f32_stem_plan(B, Hh, W)
    _claims(c, p, ("tiled", "TH", "items", "grid", "trips", "partial_band"))
    t = _stem_ops(c, dev, centre)
    exp = _expected(t["ref"], F32)
    rows = lib.cvcl_stem_conv_stats_rows(H.F32, B, Hh, W)
    assert rows == T.col_stats_rows(B * p["Ho"] * p["Wo"])
    raw, y, n = _out((B, p["Ho"], p["Wo"], 64), F32, dev, p["Wo"] * 64)
    st = torch.full((rows + 1, 2, 64), float("nan"), device=dev)
    H.check(lib.cvcl_stem_conv7x7(H.F32, H.ptr(t["x"]), H.ptr(t["wp32"]), H.ptr(y), H.ptr(st), rows, H.ptr(t["cen"]), B, Hh, W,
                                  H.stream_ptr()), "stem f32")
    torch.cuda.synchronize()
    wrong = _where_wrong(y, exp, p)
    assert not wrong, f"{c['tag']} {'tiled' if p['tiled'] else 'direct'} centre={centre}: {wrong}"
    assert torch.equal(y, exp)
    assert _tail_intact(raw, n) and bool(st[rows].isnan().all()) and bool(torch.isfinite(st[:rows]).all())
    _check_col_stats_rows(c["tag"], st[:rows], exp.reshape(-1, 64), rows)


# ---- cvcl_stem_pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [True, False], ids=["centred", "plain"])
@pytest.mark.parametrize("c", T.STEM_POOL_CASES, ids=_ids(T.STEM_POOL_CASES))
def test_stem_pool_exact(dev, c, centre):
    """stem_pool_mfma_kernel against maxpool(relu(bf16(conv - centre) * scale + shift)) in float64, rounded to bf16, and against the
    two-pass form (cvcl_stem_conv7x7, then cvcl_bn_relu_maxpool), bit for bit.  W = 228 .. 252 have 8 m-tiles per convolution row:
    the last tile's lane 15 stores one pixel past the band row, in the last band row past the band -- where -centre[0..31] used to
    lie, so that a centred stem at these widths was wrong in channels 0..31 in whatever a workgroup computed after its first item's
    last tile: a few tiles of the waves still at work, and every later item (the second-trip cases)."""
    lib = H.lib()
    B, Hh, W = c["B"], c["H"], c["W"]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    p = T.stem_pool_plan(B, Hh, W, cus)
    assert p["supported"] and lib.cvcl_stem_pool_supported(H.BF16, Hh, W)
    _claims(c, p, ("Hp", "items", "trips", "xcd", "mtiles", "partial_band", "tile_past_row"))
    t = _stem_ops(c, dev, centre)
    if centre:
        assert bool((t["cen"][:32] != 0).all())
    scale, shift = (v.to(dev) for v in T.pool_affine(64, seed=0))
    ref = T.stem_pool_reference(t["x"], t["w"], t["cen"], scale, shift)
    exp = ref.float().to(BF)
    assert float(ref.max()) > 256 and float(ref.min()) == 0 and not torch.equal(exp.double(), ref)
    raw, one, n = _out((B, p["Hp"], p["Wp"], 64), BF, dev, p["Wp"] * 64)
    H.check(lib.cvcl_stem_pool(H.BF16, H.ptr(t["x"]), H.ptr(t["wp16"]), H.ptr(scale), H.ptr(shift), H.ptr(t["cen"]), H.ptr(one), B, Hh,
                               W, H.stream_ptr()), "stem_pool")
    torch.cuda.synchronize()
    wrong = _where_wrong(one, exp, p, "pooled (b, py, px, c)")
    assert not wrong, f"{c['tag']} centre={centre}: {wrong}"
    assert torch.equal(one, exp) and _tail_intact(raw, n)
    # the two-pass form
    rows = lib.cvcl_stem_conv_stats_rows(H.BF16, B, Hh, W)
    conv = torch.empty(B, p["Ho"], p["Wo"], 64, dtype=BF, device=dev)
    st = torch.empty(rows, 2, 64, device=dev)
    two = torch.full((B, p["Hp"], p["Wp"], 64), float("nan"), dtype=BF, device=dev)
    H.check(lib.cvcl_stem_conv7x7(H.BF16, H.ptr(t["x"]), H.ptr(t["wp16"]), H.ptr(conv), H.ptr(st), rows, H.ptr(t["cen"]), B, Hh, W,
                                  H.stream_ptr()), "stem")
    H.check(lib.cvcl_bn_relu_maxpool(H.BF16, H.ptr(conv), H.ptr(scale), H.ptr(shift), H.ptr(two), B, p["Ho"], p["Wo"], 64,
                                     H.stream_ptr()), "maxpool")
    torch.cuda.synchronize()
    assert torch.equal(two, exp) and torch.equal(one, two)


def test_stem_pool_refuses_what_it_does_not_support(dev):
    assert not T.stem_pool_supported(16, 256) and not H.lib().cvcl_stem_pool_supported(H.BF16, 16, 256)
    assert not H.lib().cvcl_stem_pool_supported(H.F32, 16, 224)
    x = torch.ones(1, 3, 16, 256, device=dev)
    wp = torch.zeros(4 * 6 * 512 * 2, dtype=torch.uint8, device=dev)
    ones = torch.ones(64, device=dev)
    y = torch.full((1, 4, 64, 64), CANARY16, dtype=torch.int16, device=dev)
    rc = H.lib().cvcl_stem_pool(H.BF16, H.ptr(x), H.ptr(wp), H.ptr(ones), H.ptr(ones), None, H.ptr(y), 1, 16, 256, H.stream_ptr())
    torch.cuda.synchronize()
    assert rc == H.EINVAL and bool((y == CANARY16).all())


# ---- cvcl_bn_relu_maxpool ----------------------------------------------------------------------------------------------------------
def _run_maxpool(dev, dt, shape, batch_chunk=None):
    cd, tdt, _ = _dt(dt)
    B, Hh, W, C = shape
    p = T.maxpool_plan(B, Hh, W, C)
    x = T.int_activations(shape, Hh * 31 + W + C, dev).to(tdt)
    scale, shift = (v.to(dev) for v in T.pool_affine(C, seed=1))
    raw, y, n = _out((B, p["Ho"], p["Wo"], C), tdt, dev, p["Wo"] * C)
    H.check(H.lib().cvcl_bn_relu_maxpool(cd, H.ptr(x), H.ptr(scale), H.ptr(shift), H.ptr(y), B, Hh, W, C, H.stream_ptr()), "maxpool")
    torch.cuda.synchronize()
    step = batch_chunk or B
    saw_negative = False
    for b0 in range(0, B, step):                          # (the float64 reference of the large case in slices of the batch)
        xs = x[b0:b0 + step]
        exp = _expected(T.maxpool_reference(xs, scale, shift), tdt)
        saw_negative |= bool((xs.double() * scale.double() + shift.double() < 0).any())
        got = y[b0:b0 + step]
        w = _first_wrong(got, exp)
        if w is not None:
            _n, (b, oy, ox, ch), msg = w
            i = (((b0 + b) * T.div_up(p["Ho"], 2) + oy // 2) * p["Wo"] + ox) * (C // 8) + ch // 8
            raise AssertionError(f"{dt} {shape}: (b - {b0}, oy, ox, c) {msg}; thread index {i}, row {oy % 2} of its two, trip "
                                 f"{i // (p['grid'] * 256)} of a grid of {p['grid']}")
        assert torch.equal(got, exp)
    assert saw_negative and _tail_intact(raw, n)
    return p


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", T.MAXPOOL_SHAPES, ids=["x".join(map(str, s)) for s in T.MAXPOOL_SHAPES])
def test_bn_relu_maxpool_exact(dev, dt, shape):
    """even and odd extents, one-row and one-pixel maps, a lone last output row, C = 8 (one chunk per pixel) and C = 72"""
    assert _run_maxpool(dev, dt, shape)["trips"] == 1


def test_bn_relu_maxpool_past_the_grid_cap(dev):
    """65 x 64 x 64 x 512 in bf16 (272 MB): B * ceil(Ho / 2) * Wo * C / 8 = 2 129 920 threads' worth of work on the 8192 x 256
    threads the launcher caps the grid at, so the last 32 768 units are second trips of the grid-stride loop.  The workload's own
    stem map (256 x 112 x 112 x 64: 6.4 M units) runs in this regime on every step; nothing smaller reaches it, since the cap
    counts (pooled pixel pair, 8 channels) units and each unit reads 2 x 2 input pixels' worth of a 4-fold larger map."""
    p = _run_maxpool(dev, "bf16", T.MAXPOOL_PAST_CAP, batch_chunk=5)
    assert p["grid"] == 8192 and p["trips"] == 2


# ---- cvcl_bn_add_relu, cvcl_bn_relu_apply ----------------------------------------------------------------------------------------
def _affine_ops(dev, dt, rows, C):
    _cd, tdt, _epc = _dt(dt)
    raw = T.int_activations((rows, C), rows + C, dev).to(tdt)
    idn = T.int_activations((rows, C), rows + C + 1, dev).to(tdt)
    (s1, b1), (s2, b2) = T.pool_affine(C, 0), T.pool_affine(C, 3)
    return raw, idn, s1.to(dev), b1.to(dev), s2.to(dev), b2.to(dev)


def _check_rows(tag, y, tdt, reference, stride, epc, row_chunk=None):
    """y [rows, C] against reference(r0, r1) -> float64 [r1 - r0, C], in slices of rows"""
    rows = y.shape[0]
    step = row_chunk or rows
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        exp = _expected(reference(r0, r1), tdt)
        wrong = _where_flat(y[r0:r1], exp, epc, stride)
        assert not wrong, f"{tag} rows {r0}..{r1} (chunk and thread relative to row {r0}): {wrong}"
        assert torch.equal(y[r0:r1], exp)


def _run_bn_add_relu(dev, dt, rows, C, with_ds, row_chunk=None):
    cd, tdt, epc = _dt(dt)
    p = T.affine_plan(rows, C, epc)
    assert (p["grid"] * 256) % p["cc"] == 0
    raw, idn, s1, b1, s2, b2 = _affine_ops(dev, dt, rows, C)
    buf, out, n = _out((rows, C), tdt, dev, C)
    H.check(H.lib().cvcl_bn_add_relu(cd, H.ptr(raw), H.ptr(s1), H.ptr(b1), H.ptr(idn), H.ptr(s2) if with_ds else None,
                                     H.ptr(b2) if with_ds else None, H.ptr(out), rows, C, H.stream_ptr()), "bn_add_relu")
    torch.cuda.synchronize()

    def reference(r0, r1):
        return T.bn_add_relu_reference(raw[r0:r1], s1, b1, idn[r0:r1], s2 if with_ds else None, b2 if with_ds else None)
    _check_rows(f"bn_add_relu {dt} rows={rows} C={C} ds={with_ds}", out, tdt, reference, p["stride"], epc, row_chunk)
    assert _tail_intact(buf, n)
    return p


def _run_bn_relu_apply(dev, dt, rows, C, in_place, row_chunk=None):
    cd, tdt, epc = _dt(dt)
    p = T.affine_plan(rows, C, epc)
    raw, _idn, s1, b1, _s2, _b2 = _affine_ops(dev, dt, rows, C)
    buf, out, n = _out((rows, C), tdt, dev, C)
    if in_place:
        out.copy_(raw)
    H.check(H.lib().cvcl_bn_relu_apply(cd, H.ptr(out if in_place else raw), H.ptr(s1), H.ptr(b1), H.ptr(out), rows, C,
                                       H.stream_ptr()), "bn_relu_apply")
    torch.cuda.synchronize()

    def reference(r0, r1):
        pre = raw[r0:r1].double() * s1.double() + b1.double()
        assert row_chunk or rows * C < 64 or bool((pre < 0).any())
        return torch.relu(pre)
    _check_rows(f"bn_relu_apply {dt} rows={rows} C={C} in_place={in_place}", out, tdt, reference, p["stride"], epc, row_chunk)
    assert _tail_intact(buf, n)
    return p


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ci", range(6), ids=["Cmin", "C24", "C40", "C72", "C256", "C2048"])
def test_bn_add_relu_exact(dev, dt, ci):
    """C / EPC = 1, 3, 5, 9 chunks per row (bf16; 1, 6, 10, 18 in fp32) make the launcher round its grid to a multiple of 3, 5, 9
    so that a thread keeps its channel chunk from trip to trip; every channel has its own (scale, shift), so a thread that applied
    another chunk's affine is caught.  Rows 1, 3, 98, 1000, 1100; with and without the downsample affine on the identity."""
    C = T.affine_channels(_dt(dt)[2])[ci]
    plans = [_run_bn_add_relu(dev, dt, rows, C, ds) for rows in T.AFFINE_ROWS for ds in (False, True)]
    assert {p["mult"] for p in plans} == {[1, 3, 5, 9, 1, 1 if dt == "bf16" else 2][ci]}
    if ci in (1, 2, 3):
        assert any(p["rounded"] and p["several"] for p in plans), plans      # a grid that would not do without the rounding


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ci", range(6), ids=["Cmin", "C24", "C40", "C72", "C256", "C2048"])
def test_bn_relu_apply_exact(dev, dt, ci):
    """as above for y = relu(x * scale + shift), out of place and in place (y == x)"""
    C = T.affine_channels(_dt(dt)[2])[ci]
    for rows in T.AFFINE_ROWS:
        for in_place in (False, True):
            _run_bn_relu_apply(dev, dt, rows, C, in_place)


def test_bn_add_relu_past_the_grid_cap(dev):
    """fp32, 2 796 300 x 24 (268 MB per tensor): rows * C / 4 = 16 777 800 chunks, just above the 16384 workgroups x 1024 chunks
    at which the launcher caps the grid, which it then rounds from 16384 to 16386 (6 chunks per row).  Every thread makes two
    trips of the ``2 * stride`` loop; in the second, the threads below 4 193 352 have both chunks and the rest only the first
    (has_j == false).  The block tails of the B = 256 workload (802 816 x 256 bf16: 25.7 M chunks) run in this regime."""
    rows, C = T.AFFINE_PAST_CAP["f32"]
    p = _run_bn_add_relu(dev, "f32", rows, C, True, row_chunk=400000)
    assert p["capped"] == 16384 and p["grid"] == 16386 and p["trips"] == 2 and p["tail"] and p["tail_both"], p


def test_bn_relu_apply_past_the_grid_cap(dev):
    """bf16, 5 592 500 x 24 (268 MB): 16 777 500 chunks of 3 per row on a grid rounded from 16384 to 16386, in place"""
    rows, C = T.AFFINE_PAST_CAP["bf16"]
    p = _run_bn_relu_apply(dev, "bf16", rows, C, True, row_chunk=800000)
    assert p["capped"] == 16384 and p["grid"] == 16386 and p["trips"] == 2 and p["tail"] and p["tail_both"], p


def test_bn_add_relu_refuses_a_broken_chunk(dev):
    """C must be a multiple of the 16-byte chunk (8 bf16, 4 fp32): C = 4 is an fp32 shape and no bf16 one"""
    x = torch.zeros(2, 4, dtype=BF, device=dev)
    a = torch.ones(4, device=dev)
    rc = H.lib().cvcl_bn_add_relu(H.BF16, H.ptr(x), H.ptr(a), H.ptr(a), H.ptr(x), None, None, H.ptr(x), 2, 4, H.stream_ptr())
    assert rc == H.EINVAL
    rc = H.lib().cvcl_bn_relu_apply(H.BF16, H.ptr(x), H.ptr(a), H.ptr(a), H.ptr(x), 2, 4, H.stream_ptr())
    assert rc == H.EINVAL


# ---- cvcl_avgpool ------------------------------------------------------------------------------------------------------------------
def _run_avgpool(dev, dt, B, HW, C):
    cd, tdt, _ = _dt(dt)
    x = T.int_activations((B, HW, C), HW * 7 + C, dev, lim=64).to(tdt)
    buf, out, n = _out((B, C), F32, dev, C)
    H.check(H.lib().cvcl_avgpool(cd, H.ptr(x), H.ptr(out), B, HW, C, H.stream_ptr()), "avgpool")
    torch.cuda.synchronize()
    total = x.double().sum(dim=1)                                          # integers of at most 64 x 64: exact in fp32 in any order
    assert float(total.abs().max()) < 2 ** 24
    tot32 = total.float().cpu()
    exp = (tot32 / torch.full_like(tot32, float(HW))).to(dev)              # the fp32 quotient (IEEE division, on the host)
    w = _first_wrong(out, exp)
    assert w is None, f"avgpool {dt} B={B} HW={HW} C={C}: (b, c) {w[2]}; thread index {w[1][0] * C + w[1][1]}"
    assert torch.equal(out, exp) and _tail_intact(buf, n)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_avgpool_exact(dev, dt):
    """integer inputs: the ordered sum is exact, the result is the correctly rounded fp32 quotient sum / HW"""
    for HW in T.AVGPOOL_HW:
        for C in T.AVGPOOL_C:
            _run_avgpool(dev, dt, 3, HW, C)
    B, HW, C = T.AVGPOOL_PAST_CAP
    p = T.avgpool_plan(B, C)
    assert p["grid"] == 4096 and p["trips"] == 2                            # B * C past the 4096 x 256 threads of the grid
    _run_avgpool(dev, dt, B, HW, C)


# ---- cvcl_col_stats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("rows", T.COL_STATS_ROWS)
def test_col_stats_exact(dev, dt, rows):
    """integer inputs within +-8: every partial row is exact.  Fewer rows than row slices, one block, several blocks, and 65543
    rows on the 256 blocks the grid is capped at (grid-stride trips; two blocks get a 65th group); C = 100 and 192 leave the last
    64-channel block of columns partly or wholly in use (``ch < C``)."""
    cd, tdt, _ = _dt(dt)
    g = H.lib().cvcl_col_stats_rows(rows)
    assert g == T.col_stats_rows(rows) and (rows < 65536 or (g == 256 and rows > 256 * 4 * 64))
    for C in T.COL_STATS_C:
        x = T.int_activations((rows, C), rows + C, dev, lim=8).to(tdt)
        st = torch.full((g + 1, 2, C), float("nan"), device=dev)
        H.check(H.lib().cvcl_col_stats(cd, H.ptr(x), rows, C, H.ptr(st), g, H.stream_ptr()), "col_stats")
        torch.cuda.synchronize()
        assert bool(st[g].isnan().all()), "wrote behind the statistics rows"
        assert bool(torch.isfinite(st[:g]).all()), "a statistics row was left unwritten"
        _check_col_stats_rows(f"col_stats {dt} rows={rows} C={C}", st[:g], x, g)
        st.fill_(float("nan"))
        rc = H.lib().cvcl_col_stats(cd, H.ptr(x), rows, C, H.ptr(st), g - 1, H.stream_ptr())
        torch.cuda.synchronize()
        assert rc == H.EINVAL and "stats_rows" in H.lib().cvcl_last_error().decode() and bool(st.isnan().all())


# ---- cvcl_bn_finalize, cvcl_bn_eval_affine ---------------------------------------------------------------------------------------
PAD = 16


def _padded(v, fill):
    """[C] -> a buffer of C + PAD with ``fill`` behind the C values, and its first C as a view"""
    buf = torch.full((v.shape[0] + PAD,), fill, dtype=v.dtype, device=v.device)
    buf[:v.shape[0]] = v
    return buf, buf[:v.shape[0]]


def _finalize(t, rows, count, C, dev):
    """one cvcl_bn_finalize launch on the operands ``t``; every [C] output sits in a buffer with a canary tail"""
    out = {}
    for k in ("scale", "shift"):
        out[k + "_buf"], out[k] = _padded(torch.full((C,), float("nan"), device=dev), float("nan"))
    out["rm_buf"], out["rm"] = _padded(t["rm"].clone(), 777.0)
    out["rv_buf"], out["rv"] = _padded(t["rv"].clone(), 777.0)
    out["nbt"] = torch.tensor([41, -5], dtype=torch.int64, device=dev)
    H.check(H.lib().cvcl_bn_finalize(H.ptr(t["stats"]), rows, count, H.ptr(t["gamma"]), H.ptr(t["beta"]), H.ptr(out["rm"]),
                                     H.ptr(out["rv"]), H.ptr(out["nbt"]), t["momentum"], t["eps"], H.ptr(out["scale"]),
                                     H.ptr(out["shift"]), H.ptr(t["centre"]), C, H.stream_ptr()), "bn_finalize")
    torch.cuda.synchronize()
    assert out["nbt"].tolist() == [42, -5]
    for k in ("scale", "shift"):
        assert bool(out[k + "_buf"][C:].isnan().all()), f"wrote behind {k}"
    assert bool((out["rm_buf"][C:] == 777.0).all()) and bool((out["rv_buf"][C:] == 777.0).all()), "wrote behind the running statistics"
    return out


@pytest.mark.parametrize("rows", T.FINALIZE_ROWS)
def test_bn_finalize_exact(dev, rows):
    """Hand-made partial rows whose float64 sums are exactly count * mean and count * (var + mean^2), var + eps a power of four
    (eps = 1/4), dyadic gamma / beta / running statistics / centres, momentum 1/2: scale, shift, running_mean and
    num_batches_tracked must be the float64 values, running_var the fp32 rounding of m * fp32(unbiased) + (1 - m) * old.  1 .. 1025
    partial rows: fewer than the 64 row slices, a second trip of the slice loop (r0 += 512) from 513 on, a third at 1025; C = 1, 15,
    17 leave lanes of a 16-channel workgroup idle (canary behind every output); count = 1 has no unbiased correction; and
    E[x^2] - mean^2 = -1/64 must clamp to var = 0."""
    for C in T.FINALIZE_C:
        for count in T.FINALIZE_COUNTS:
            for centre, neg in ((True, False), (False, False), (True, True)):
                t = T.finalize_exact_inputs(rows, C, count, rows * 7 + C + count, dev, centre=centre, negative_var=neg)
                r = T.bn_finalize_reference(t["stats"], count, t["gamma"], t["beta"], t["rm"], t["rv"], t["momentum"], t["eps"],
                                            t["centre"])
                assert torch.equal(r["mean"], t["mean"]) and torch.equal(r["var"], t["var"])
                if neg:
                    s = t["stats"].double().sum(dim=0)
                    assert bool((s[1] / torch.full_like(s[1], count) - r["mean"] * r["mean"] < 0).all()) and not bool(r["var"].any())
                out = _finalize(t, rows, count, C, dev)
                tag = f"rows={rows} C={C} count={count} centre={centre} negative_var={neg}"
                for k, want in (("scale", r["scale"]), ("shift", r["shift"]), ("rm", r["running_mean"])):
                    assert torch.equal(want.float().double(), want)              # (fp32 holds the float64 value)
                    bad = (out[k].double() != want).nonzero().flatten().tolist()
                    assert not bad, f"{tag}: {k} wrong in channels {bad[:16]}: {out[k][bad[:4]].tolist()} != {want[bad[:4]].tolist()}"
                bad = (out["rv"] != r["running_var_2"].float()).nonzero().flatten().tolist()
                assert not bad, f"{tag}: running_var wrong in channels {bad[:16]}"
                if count <= 2:
                    assert torch.equal(r["running_var_2"], r["running_var"]) and torch.equal(out["rv"].double(), r["running_var"])


def _random_finalize_inputs(rows, C, per_row, seed, dev, centre):
    """partial rows of a random tensor: row r holds the fp32-rounded float64 sums of ``per_row`` samples per channel; channel means
    within a few standard deviations of 0, standard deviations 0.1 .. 3"""
    g = torch.Generator(device=dev).manual_seed(seed)
    mu = torch.randn(C, generator=g, device=dev, dtype=F64) * 2
    sd = torch.rand(C, generator=g, device=dev, dtype=F64) * 2.9 + 0.1
    stats = torch.empty(rows, 2, C, device=dev)
    for r0 in range(0, rows, 64):
        r1 = min(rows, r0 + 64)
        x = (torch.randn(r1 - r0, per_row, C, generator=g, device=dev, dtype=F64) * sd + mu).float().double()
        stats[r0:r1, 0], stats[r0:r1, 1] = x.sum(dim=1).float(), (x * x).sum(dim=1).float()

    def rnd(lo, hi):
        return (torch.rand(C, generator=g, device=dev) * (hi - lo) + lo)
    cen = (mu.float() + 0.05 * rnd(-1, 1)) if centre else None
    if centre:                                           # the statistics are those of the stored tensor y - c
        n = per_row
        s, q = stats[:, 0].double(), stats[:, 1].double()
        c64 = cen.double()
        stats[:, 1] = (q - 2 * c64 * s + n * c64 * c64).float()
        stats[:, 0] = (s - n * c64).float()
    return dict(stats=stats, gamma=rnd(0.5, 1.5), beta=rnd(-1, 1), rm=rnd(-1, 1), rv=rnd(0.5, 1.5), centre=cen, eps=1e-5, momentum=0.1)


@pytest.mark.parametrize("rows,C,per_row", [(513, 100, 24), (65, 17, 193), (1025, 2048, 12), (1, 64, 12544)])
@pytest.mark.parametrize("centre", [True, False], ids=["centred", "plain"])
def test_bn_finalize_random_within_the_derived_bounds(dev, rows, C, per_row, centre):
    """Random statistics, eps = 1e-5, momentum = 0.1, per channel against float64.  With u = 2^-24 (the unit roundoff of fp32; one
    ulp is at most 2 u relative) the kernel's operation sequence gives:

      scale = gamma / sqrtf((float)var + eps)
        (float)var: relative error u; + eps: the sum inherits at most u and its own rounding adds u, 2 u on var + eps; the
        square root halves that to u; sqrtf itself is within 1 ulp (HIP math API accuracy table), 2 u; the division is correctly
        rounded unless fast-math is on, and within 1 ulp = 2 u in any case.            |scale - ref| <= 5 u |ref|
      shift = beta - (float)mean * scale
        (float)mean: u; scale: 5 u; the product's rounding: u -- 7 u of |mean * scale|; the subtraction's rounding: u of the
        result.                                                                    |shift - ref| <= 7 u |mean scale| + u |ref|
      running = fmaf(m, (float)new, (1 - m) * old), 1 - m formed in fp32 (the reference uses the same fp32 value)
        (float)new: u of |m new|; the product (1 - m) old: u of itself; the fused multiply-add: u of the result.
                                                                  |running - ref| <= u (|m new| + |(1 - m) old| + |ref|)

    var, mean, unbiased and mean + centre are float64 in the kernel as in the reference; the two add the partial rows in another
    order, which moves var by about 2^-53 E[x^2] / var relative: below 1e-12 here.  Each bound carries a factor 1.01 for that and for
    the second-order terms.  Largest errors observed on an MI355X, as fractions of these bounds: scale 0.43, shift 0.93,
    running_mean 0.81, running_var 0.85 (a correctly rounded last operation alone comes to within u of its result: up to 1)."""
    count = rows * per_row
    t = _random_finalize_inputs(rows, C, per_row, rows + C, dev, centre)
    r = T.bn_finalize_reference(t["stats"], count, t["gamma"], t["beta"], t["rm"], t["rv"], t["momentum"], t["eps"], t["centre"])
    assert float((r["mean"] * r["mean"] / r["var"]).max()) < 1e4 and float(r["var"].min()) > 0
    out = _finalize(t, rows, count, C, dev)
    bounds = dict(scale=5 * U * r["scale"].abs(),
                  shift=7 * U * (r["mean"] * r["scale"]).abs() + U * r["shift"].abs(),
                  rm=U * ((r["m"] * r["true_mean"]).abs() + (r["one_m"] * t["rm"].double()).abs() + r["running_mean"].abs()),
                  rv=U * ((r["m"] * r["unbiased"]).abs() + (r["one_m"] * t["rv"].double()).abs() + r["running_var"].abs()))
    want = dict(scale=r["scale"], shift=r["shift"], rm=r["running_mean"], rv=r["running_var"])
    for k, bound in bounds.items():
        err = (out[k].double() - want[k]).abs()
        print(f"bn_finalize rows={rows} C={C} centre={centre}: {k} largest error / bound = {float((err / bound).max()):.3f}")
        bad = (~(err <= 1.01 * bound)).nonzero().flatten().tolist()
        assert not bad, f"{k} outside its bound in channels {bad[:16]}: error / bound = {(err / bound)[bad[:4]].tolist()}"


def _eval_affine(t, C, dev):
    scale_buf, scale = _padded(torch.full((C,), float("nan"), device=dev), float("nan"))
    shift_buf, shift = _padded(torch.full((C,), float("nan"), device=dev), float("nan"))
    H.check(H.lib().cvcl_bn_eval_affine(H.ptr(t["gamma"]), H.ptr(t["beta"]), H.ptr(t["rm"]), H.ptr(t["rv"]), t["eps"], H.ptr(scale),
                                        H.ptr(shift), H.ptr(t["centre"]), C, H.stream_ptr()), "bn_eval_affine")
    torch.cuda.synchronize()
    assert bool(scale_buf[C:].isnan().all()) and bool(shift_buf[C:].isnan().all()), "wrote behind its outputs"
    return scale, shift


@pytest.mark.parametrize("C", [1, 15, 16, 17, 64, 255, 256, 257, 2048])
def test_bn_eval_affine_exact_and_random(dev, C):
    """exact: running_var + eps a power of four (eps = 1/4), everything else dyadic -- scale and shift are the float64 values.
    random (eps = 1e-5): scale = gamma / sqrtf(rv + eps): the sum's rounding u, halved by the root; sqrtf 2 u; the division 2 u:
    |scale - ref| <= 4.5 u |ref|.  shift = beta - (rm - centre) * scale: the difference's rounding u, scale 4.5 u, the product's
    rounding u: 6.5 u of |(rm - centre) scale|, and u of the result for the subtraction.  Factor 1.01 for second-order terms.
    Largest errors observed on an MI355X, as fractions of these bounds: scale 0.39, shift 0.71.
    C around 256 crosses the one-workgroup boundary of the launch."""
    for centre in (True, False):
        t = T.finalize_exact_inputs(1, C, 2, C, dev, centre=centre)
        t["rv"] = t["var"].float()                                               # {0, 0.75, 3.75, 15.75}
        r = T.bn_eval_affine_reference(t["gamma"], t["beta"], t["rm"], t["rv"], 0.25, t["centre"])
        scale, shift = _eval_affine(t, C, dev)
        assert torch.equal(scale.double(), r["scale"]) and torch.equal(shift.double(), r["shift"]), (C, centre)
        t = _random_finalize_inputs(1, C, 2, C, dev, centre)
        r = T.bn_eval_affine_reference(t["gamma"], t["beta"], t["rm"], t["rv"], 1e-5, t["centre"])
        scale, shift = _eval_affine(t, C, dev)
        e_sc = (scale.double() - r["scale"]).abs() / (4.5 * U * r["scale"].abs())
        e_sh = (shift.double() - r["shift"]).abs() / (6.5 * U * (r["d"] * r["scale"]).abs() + U * r["shift"].abs())
        print(f"bn_eval_affine C={C} centre={centre}: largest error / bound: scale {float(e_sc.max()):.3f}, shift {float(e_sh.max()):.3f}")
        assert bool((e_sc <= 1.01).all()) and bool((e_sh <= 1.01).all()), (C, centre, float(e_sc.max()), float(e_sh.max()))


# ---- cvcl_pack_conv_weight(STEM7) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_weight_packer_writes_its_bytes_and_no_more(dev, dt):
    """cvcl_packed_weight_bytes bytes of a canary-filled buffer are all written and the 256 behind them are not (the values are
    covered by the exact stem results); fp32 keeps the OIHW layout, so there the packed weights are the weights"""
    cd, _tdt, _ = _dt(dt)
    _x, w, _cen = T.stem_inputs(1, 8, 16, 9)
    packed = _pack_stem(cd, w, dev)
    if dt == "f32":
        assert torch.equal(packed.view(F32).view(64, 3, 7, 7), w.to(dev))
    else:
        vals = packed.view(BF).float()
        assert float(vals.abs().max()) <= 2 and torch.equal(vals, vals.round())
        assert int((vals != 0).sum()) == int((w != 0).sum())                     # every weight once, zeros in the padded k
