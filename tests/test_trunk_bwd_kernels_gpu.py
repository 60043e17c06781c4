"""GPU: the backward-side kernels of the ResNeXt trunk (csrc/trunk_bwd.hip), one by one through the C ABI, in fp32 and bf16,
exactly, against float64 (tests/trunk_bwd_cases.py): cvcl_bn_apply, cvcl_bn_bwd in its three modes, cvcl_bn_batch_moments,
cvcl_maxpool3x3s2_idx in both directions, cvcl_avgpool_bwd, cvcl_zero_stuff2, cvcl_add, cvcl_relu_mask, cvcl_gconv_weight_dgrad,
cvcl_transpose and cvcl_conv_wgrad_direct.

The operands are small integers, halves and powers of two, on which every fp32 product, sum and fmaf is exact in any order
(test_trunk_bwd_reference_host.py proves it case by case): an fp32 kernel must return the float64 result and a bf16 kernel its bf16
rounding, bit for bit but for the sign of a zero.  Every case first asserts, from the launcher restatements and from
cvcl_bn_bwd_partial_rows, the regime it was chosen for.  Outputs carry a canary tail (NaN for fp32, the 0x7B7B pattern for bf16);
scratch rows start as NaN and exactly the announced number must have been written.  A failure names the first wrong element and the
chunk, thread and trip that computed it.

The only comparisons that are not equalities: the coefficients and dx of cvcl_bn_bwd where the row count is no power of two
(test_bn_bwd_ragged_within_the_derived_bound derives the bound), rstd at a count that is no power of two (one fp32 ulp), and the
quotient of cvcl_avgpool_bwd, which is the host's fp32 IEEE quotient."""
import pytest
import torch
import torch.nn.functional as F

from multimodal import _hip as H

import trunk_bwd_cases as T

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
CANARY16 = 0x7B7B                                     # bit pattern of a bf16 canary (a finite value no case produces)
CANARY8 = 0xA5                                        # of an arg-max byte (no window code)
NAN = float("nan")


def _ids(cases):
    return [c["tag"] for c in cases]


def _dt(dt):
    return (H.BF16, BF, 8) if dt == "bf16" else (H.F32, F32, 4)


def _out(shape, tdt, dev, tail):
    """an output tensor of ``shape`` with ``tail`` canary elements behind it -> (whole buffer, view, n)"""
    n = 1
    for s in shape:
        n *= s
    if tdt == BF:
        raw = torch.full((n + tail,), CANARY16, dtype=torch.int16, device=dev)
        return raw, raw[:n].view(BF).view(shape), n
    raw = torch.full((n + tail,), NAN, dtype=tdt, device=dev)
    return raw, raw[:n].view(shape), n


def _tail_intact(raw, n):
    return bool((raw[n:] == CANARY16).all()) if raw.dtype == torch.int16 else bool(raw[n:].isnan().all())


def _untouched(raw):
    return _tail_intact(raw, 0)


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


def _where(y, exp, chunk, stride, per_trip=1, offset=0):
    """y, exp [.., C] of a kernel whose thread i0 takes the ``chunk``-element pieces i0, i0 + stride, .., ``per_trip`` of them per
    trip of its loop; ``offset``: elements in front of y[0] (a slice of a larger tensor).  '' where nothing is wrong."""
    w = _first_wrong(y, exp)
    if w is None:
        return ""
    _n, idx, msg = w
    flat = offset + sum(i * s for i, s in zip(idx, y.stride()))
    i = flat // chunk
    return (f"{msg}; chunk {i}, thread {i % stride}, trip {i // (stride * per_trip)}"
            + (f" (chunk {(i // stride) % per_trip} of its {per_trip})" if per_trip > 1 else "") + f" at a stride of {stride}")


def _check(tag, y, ref64, tdt, chunk, stride, per_trip=1, offset=0):
    exp = _expected(ref64, tdt)
    wrong = _where(y, exp, chunk, stride, per_trip, offset)
    assert not wrong, f"{tag}: {wrong}"
    assert y.dtype == exp.dtype and y.shape == exp.shape and torch.equal(y, exp)              # (equal but for the sign of a zero)


def _vec(C, dev, pad=16):
    """a NaN-filled [C] fp32 output with ``pad`` canary elements behind it -> (buffer, view)"""
    buf = torch.full((C + pad,), NAN, device=dev)
    return buf, buf[:C]


def _vec_exact(tag, got, want64):
    assert T.is_f32(want64), tag
    bad = ((got.double() != want64) | got.isnan()).nonzero().flatten().tolist()
    assert not bad, f"{tag}: wrong in channels {bad[:16]}: {got[bad[:4]].tolist()} != {want64[bad[:4]].tolist()}"


# ---- cvcl_bn_apply -----------------------------------------------------------------------------------------------------------------
def _run_bn_apply(dev, dt, rows, C, relu, row_chunk=None):
    cd, tdt, epc = _dt(dt)
    assert T.bn_apply_supported(C, epc)
    p = T.bn_apply_plan(rows, C, epc)
    assert p["fixed_chunk"]
    x = T.int_activations((rows, C), rows + C, dev).to(tdt)
    scale, shift = (v.to(dev) for v in T.pool_affine(C, seed=2))
    buf, y, n = _out((rows, C), tdt, dev, C)
    H.check(H.lib().cvcl_bn_apply(cd, H.ptr(x), H.ptr(scale), H.ptr(shift), H.ptr(y), rows, C, relu, H.stream_ptr()), "bn_apply")
    torch.cuda.synchronize()
    step = row_chunk or rows
    saw_negative = False
    for r0 in range(0, rows, step):                       # (the float64 reference of the large case in row slices)
        r1 = min(rows, r0 + step)
        ref = T.bn_apply_reference(x[r0:r1], scale, shift, relu)
        saw_negative |= bool((ref < 0).any())
        _check(f"bn_apply {dt} rows={rows} C={C} relu={relu} rows {r0}..{r1}", y[r0:r1], ref, tdt, epc, p["stride"], offset=r0 * C)
    assert _tail_intact(buf, n) and (saw_negative == (not relu) or rows * C < 64)
    return p


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cc", T.BN_APPLY_CC)
def test_bn_apply_exact(dev, dt, cc):
    """y = x * scale + shift (+ReLU): 1, 8, 256 and 768 chunks per row -- 768 makes the launcher round its grid to a multiple of 3 so
    that a thread keeps its channel chunk; every channel has its own (scale, shift)"""
    epc = _dt(dt)[2]
    plans = [_run_bn_apply(dev, dt, rows, cc * epc, relu) for rows in T.AFFINE_ROWS for relu in (0, 1)]
    if cc == 768:
        assert all(p["grid"] % 3 == 0 for p in plans) and any(p["rounded"] for p in plans)


def test_bn_apply_past_the_grid_cap(dev):
    """bf16, 21 846 x 6144 (268 MB): 16 777 728 chunks of 768 per row, on a grid capped at 16384 and rounded to 16386; every thread
    makes four trips of the grid-stride loop with the (scale, shift) it loaded once"""
    rows, C = T.BN_APPLY_PAST_CAP
    p = _run_bn_apply(dev, "bf16", rows, C, 1, row_chunk=2000)
    assert p["total"] == 16777728 and p["capped"] == 16384 and p["grid"] == 16386 and p["trips"] == 4, p


# ---- cvcl_bn_bwd -------------------------------------------------------------------------------------------------------------------
EXTRA_PARTIAL = 3


def _bn_bwd(dev, dt, rows, C, mode, t, partial_rows=None, C_arg=None, mode_arg=None, drop=(), mean_offset=0):
    """one cvcl_bn_bwd launch on the operands ``t`` (T.bn_bwd_inputs on the device); every output and scratch buffer starts as a
    canary.  -> (rc, dict of buffers).  The keyword arguments break one argument each, for the refusals."""
    cd, tdt, _epc = _dt(dt)
    lib = H.lib()
    prow = lib.cvcl_bn_bwd_partial_rows(cd, rows, C)
    o = dict(prow=prow)
    o["partial"] = torch.full((prow + EXTRA_PARTIAL, 2, C), NAN, device=dev)
    o["coef_buf"], o["coef"], _ = _out((3, C), F32, dev, C)
    o["dgamma_buf"], o["dgamma"] = _vec(C, dev)
    o["dbeta_buf"], o["dbeta"] = _vec(C, dev)
    o["dx_buf"], o["dx"], o["n"] = _out((rows, C), tdt, dev, C)
    o["g_buf"], o["g"], _ = _out((rows, C), tdt, dev, C)
    x, dy, out = t["x"].to(tdt), t["dy"].to(tdt), t["out"].to(tdt)
    mean = t["mean"]
    if mean_offset:
        o["mean_shifted"] = torch.cat([torch.zeros(mean_offset, device=dev), mean, torch.zeros(4 - mean_offset, device=dev)])
        mean_ptr = H.ptr(o["mean_shifted"]) + 4 * mean_offset
    else:
        mean_ptr = H.ptr(mean)
    m = mode if mode_arg is None else mode_arg
    args = dict(out=H.ptr(out) if mode == 2 else None, scale=H.ptr(t["scale"]) if mode == 1 else None,
                shift=H.ptr(t["shift"]) if mode == 1 else None)
    for k in drop:
        args[k] = None
    rc = lib.cvcl_bn_bwd(cd, m, H.ptr(x), args["out"], H.ptr(dy), args["scale"], args["shift"], mean_ptr, H.ptr(t["rstd"]),
                         H.ptr(t["gamma"]), H.ptr(o["dgamma"]), H.ptr(o["dbeta"]), H.ptr(o["dx"]), H.ptr(o["g"]), rows,
                         C if C_arg is None else C_arg, H.ptr(o["partial"]), prow + EXTRA_PARTIAL if partial_rows is None else partial_rows,
                         H.ptr(o["coef"]), H.stream_ptr())
    torch.cuda.synchronize()
    return rc, o


def _bn_bwd_common(tag, dev, dt, rows, C, mode, t, p):
    """launch, and check what is exact in every case: the tails, the partial rows (exactly prow of them written, each the exact
    sum of its rows), dbeta, dgamma, k1 and g_out.  -> (buffers, reference)"""
    _cd, tdt, epc = _dt(dt)
    rc, o = _bn_bwd(dev, dt, rows, C, mode, t)
    assert rc == 0, H.lib().cvcl_last_error().decode()
    assert o["prow"] == p["g"], (tag, o["prow"], p)
    r = T.bn_bwd_reference(mode, t["x"], t["out"], t["dy"], t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"])
    for k in ("coef", "dgamma", "dbeta", "dx", "g"):
        assert _tail_intact(o[k + "_buf"], o[k].numel()), f"{tag}: wrote behind {k}"
    prow = o["prow"]
    assert bool(o["partial"][prow:].isnan().all()), f"{tag}: wrote behind the {prow} partial rows"
    assert bool(torch.isfinite(o["partial"][:prow]).all()), f"{tag}: a partial row was left unwritten"
    want = T.bn_bwd_partials(r, t, p)
    assert T.is_f32(want)
    bad = (o["partial"][:prow].double() != want).nonzero()
    assert not len(bad), (f"{tag}: {len(bad)} partial sums wrong; first at (workgroup bx, sum g | sum g xhat, channel) = {bad[0].tolist()}"
                          f" (channel chunk {int(bad[0][2]) // epc}, by = {int(bad[0][2]) // epc // p['ccb']})")
    _vec_exact(f"{tag}: dbeta", o["dbeta"], r["dbeta"])
    _vec_exact(f"{tag}: dgamma", o["dgamma"], r["dgamma"])
    _vec_exact(f"{tag}: coef k1", o["coef"][0], r["k1"])
    _check(f"{tag}: g_out", o["g"], r["g"], tdt, epc, p["astride"], per_trip=2)
    return o, r


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("c", T.BN_BWD_EXACT, ids=_ids(T.BN_BWD_EXACT))
def test_bn_bwd_exact(dev, c, mode):
    """rows a power of two, gamma and rstd powers of two, integer mean, x and dy: the partial rows, dbeta, dgamma, the three
    coefficients, dx and g_out bit for bit.  Mode 1 uses the forward's own affine with pre-activations that are exactly 0 (masked:
    ``> 0``), mode 2 an ``out`` of +0, -0 and positives.  The shapes: row lanes without a row, a partial group of the 4-row unroll,
    several workgroups and trips of the row loop, one row lane on a capped grid whose finalize reads 8 partial rows per slice, and
    fp32 with two channel blocks."""
    _cd, tdt, epc = _dt(c["dt"])
    rows, C = c["rows"], c["C"]
    p = T.bn_bwd_plan(epc, rows, C)
    for k in T.BN_BWD_CLAIMS:
        if k in c:
            assert p[k] == c[k], (c["tag"], k, p)
    t = T.bn_bwd_inputs(rows, C, rows + C, dev)
    tag = f"{c['tag']} mode {mode}"
    o, r = _bn_bwd_common(tag, dev, c["dt"], rows, C, mode, t, p)
    assert not T.bn_bwd_exactness(t, r, p)
    _vec_exact(f"{tag}: coef k2", o["coef"][1], r["k2"])
    _vec_exact(f"{tag}: coef k3", o["coef"][2], r["k3"])
    _check(f"{tag}: dx", o["dx"], r["dx"], tdt, epc, p["astride"], per_trip=2)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ci", range(4), ids=["Cmin", "C64", "C256", "C2048"])
def test_bn_bwd_ragged_within_the_derived_bound(dev, dt, ci):
    """rows in 3, 98, 1000, 1100, 4097: 1 / n is no fp32 number, so the coefficients and dx are rounded; the partial rows, dbeta,
    dgamma, k1 and g_out are exact as before.  With u = 2^-24 the kernel's operation sequence (built without fp contraction) is

      inv_n = 1.f / (float)n              (float)n exact; the division within 1 ulp = 2 u (u where it is correctly rounded)
      k1    = gamma * rstd                exact (powers of two)
      k2    = ((-k1 * rstd) * dgamma) * inv_n        the first two products exact (powers of two), the last rounds: inv_n's 2 u
                                                     and 1 u                                      |k2 - K2| <= 3 u |K2|
      k3    = (-k1 * dbeta) * inv_n  -  k2 * mean    A = -k1 dbeta / n carries 2 u + 1 u; k2 * mean carries k2's 3 u and the
                                                     product's u; the subtraction rounds once more, u of the result <= u (|A| +
                                                     |K2 mean|)                      |k3 - K3| <= 5 u (|A| + |K2 mean|)
      dx    = fma(k1, g, fma(k2, x, k3))             the inner fma rounds once, the outer once

    so of the four terms of dx = k1 g + K2 x + A - K2 mean, k1 g carries 1 rounding, K2 x 3 + 2 = 5 u, A 3 + 1 (k3's subtraction) +
    2 = 6 u, and K2 mean 4 + 1 + 2 = 7 u: seven roundings on the worst term, eight with the double -> float casts of dbeta and
    dgamma counted (exact here).  The bound is 8 u (|k1 g| + |K2 x| + |A| + |K2 mean|), the eighth u covering every second-order
    term; bf16 adds the rounding of the stored value, 2^-8 of (|dx| + that bound).  A masked or mixed-up element is wrong by a whole
    term: orders of magnitude more.  Largest errors observed on an MI355X, as fractions of these bounds: k2 0.57, k3 0.60, dx 0.39
    in fp32 and 1.00 in bf16 (the stored value's own half ulp)."""
    cd, tdt, epc = _dt(dt)
    C = T.bn_bwd_ragged_channels(dt)[ci]
    for rows in T.BN_BWD_RAGGED_ROWS:
        p = T.bn_bwd_plan(epc, rows, C)
        t = T.bn_bwd_inputs(rows, C, rows + C, dev)
        for mode in (0, 1, 2):
            tag = f"{dt} rows={rows} C={C} mode {mode}"
            o, r = _bn_bwd_common(tag, dev, dt, rows, C, mode, t, p)
            e2 = (o["coef"][1].double() - r["k2"]).abs()
            e3 = (o["coef"][2].double() - r["k3"]).abs()
            b2, b3 = 3 * T.U * r["k2"].abs(), 5 * T.U * (r["a0"].abs() + r["k2mean"].abs())
            bound = 8 * T.U * r["magnitude"]
            if tdt == BF:
                bound = bound + T.U16 * (r["dx"].abs() + bound)
            err = (o["dx"].double() - r["dx"]).abs()
            worst = float((err / bound.clamp(min=1e-300)).max())
            print(f"bn_bwd {tag}: largest error / bound: k2 {float((e2 / b2.clamp(min=1e-300)).max()):.3f}, "
                  f"k3 {float((e3 / b3.clamp(min=1e-300)).max()):.3f}, dx {worst:.3f}")
            assert bool((e2 <= b2).all()), f"{tag}: k2 outside its bound in channels {(~(e2 <= b2)).nonzero().flatten().tolist()[:16]}"
            assert bool((e3 <= b3).all()), f"{tag}: k3 outside its bound in channels {(~(e3 <= b3)).nonzero().flatten().tolist()[:16]}"
            bad = ~(err <= bound)
            if bool(bad.any()):
                rr, ch = bad.nonzero()[0].tolist()
                i = (rr * C + ch) // epc
                raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} dx outside the bound; first at ({rr}, {ch}): got "
                                     f"{float(o['dx'][rr, ch])}, want {float(r['dx'][rr, ch])}, bound {float(bound[rr, ch])}; chunk {i}, "
                                     f"thread {i % p['astride']}, trip {i // (2 * p['astride'])} at a stride of {p['astride']}")


def _bn_bwd_untouched(o):
    return all(_untouched(o[k]) for k in ("coef_buf", "dgamma_buf", "dbeta_buf", "dx_buf", "g_buf")) and bool(o["partial"].isnan().all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_bwd_refusals_launch_nothing(dev, dt):
    """each returns CVCL_EINVAL and leaves every output and scratch buffer at its canary: a C that is no multiple of the chunk, a
    C / chunk that is no power of two, a mode outside 0..2, mode 1 without scale or shift, mode 2 without out, partial_rows one too
    small, and a mean one float off its 16-byte alignment"""
    _cd, _tdt, epc = _dt(dt)
    rows, C = 1024, 8 * epc
    t = T.bn_bwd_inputs(rows, C, 1, dev)
    rc, o = _bn_bwd(dev, dt, rows, C, 2, t)                  # the operands are good ones
    assert rc == 0 and o["prow"] == 4 and not _bn_bwd_untouched(o)
    breaks = [dict(C_arg=C - epc // 2), dict(C_arg=3 * epc), dict(mode_arg=3), dict(mode_arg=-1), dict(partial_rows=o["prow"] - 1),
              dict(mean_offset=1)]
    for mode, kw in [(0, b) for b in breaks] + [(1, dict(drop=("scale",))), (1, dict(drop=("shift",))), (2, dict(drop=("out",)))]:
        rc, o = _bn_bwd(dev, dt, rows, C, mode, t, **kw)
        assert rc == H.EINVAL and "cvcl_bn_bwd" in H.lib().cvcl_last_error().decode(), (mode, kw, rc)
        assert _bn_bwd_untouched(o), (mode, kw)
    assert not T.bn_bwd_supported(3 * epc, epc) and not T.bn_bwd_supported(C - epc // 2, epc)


# ---- cvcl_bn_batch_moments ----------------------------------------------------------------------------------------------------------
def _moments(dev, stats, rows, count, eps, C, centre):
    mean_buf, mean = _vec(C, dev)
    rstd_buf, rstd = _vec(C, dev)
    cen_buf = cen = None
    if centre is not None:
        cen_buf = torch.full((C + 16,), 777.0, device=dev)
        cen = cen_buf[:C]
        cen.copy_(centre)
    H.check(H.lib().cvcl_bn_batch_moments(H.ptr(stats), rows, count, eps, H.ptr(mean), H.ptr(rstd), H.ptr(cen), C, H.stream_ptr()),
            "bn_batch_moments")
    torch.cuda.synchronize()
    assert bool(mean_buf[C:].isnan().all()) and bool(rstd_buf[C:].isnan().all()), "wrote behind mean / rstd"
    assert cen_buf is None or bool((cen_buf[C:] == 777.0).all()), "wrote behind centre_track"
    return mean, rstd, cen


@pytest.mark.parametrize("rows", T.MOMENTS_ROWS)
def test_bn_batch_moments_exact(dev, rows):
    """statistics rows whose float64 sums are exactly count * mean and count * (var + mean^2), count = 4096: mean, rstd and the
    updated centre must be the float64 formula (biased variance, eps as (double)(float)eps) rounded to fp32, bit for bit -- with
    eps = 1/4, where var + eps is a power of four and rstd a power of two, and with the workload's 1e-5, a real square root.
    1 .. 513 statistics rows: fewer than the 8 row slices, 8, 9, and 65 reads per slice; C = 4 and 100 leave lanes of a 32-channel
    workgroup idle.  One variant has the sum of squares lowered so that E[x^2] - mean^2 = -1/64 must clamp to var = 0; one a count
    of 12544, no power of two: within one fp32 ulp."""
    for C in T.MOMENTS_C:
        for count, neg in ((T.MOMENTS_COUNT, False), (T.MOMENTS_COUNT, True), (T.MOMENTS_RAGGED_COUNT, False)):
            t = T.moments_inputs(rows, C, count, rows * 5 + C + count, dev, negative_var=neg)
            for eps in (0.25, 1e-5):
                for with_centre in (True, False):
                    tag = f"rows={rows} C={C} count={count} negative_var={neg} eps={eps} centre={with_centre}"
                    r = T.bn_moments_reference(t["stats"], count, eps, t["centre"])
                    assert bool((r["raw_var"] < 0).all()) == neg and (not neg or not bool(r["var"].any()))
                    mean, rstd, cen = _moments(dev, t["stats"], rows, count, eps, C, t["centre"] if with_centre else None)
                    _vec_exact(f"{tag}: mean", mean.cpu(), r["mean"])
                    want = r["rstd"].float()
                    if count == T.MOMENTS_COUNT:
                        bad = (rstd.cpu() != want).nonzero().flatten().tolist()
                        assert not bad, f"{tag}: rstd wrong in channels {bad[:16]}: {rstd.cpu()[bad[:4]].tolist()} != {want[bad[:4]].tolist()}"
                    else:
                        ulp = torch.nextafter(want, torch.full_like(want, float("inf"))) - want
                        assert bool(((rstd.cpu() - want).abs() <= ulp).all()), tag
                    if with_centre:
                        _vec_exact(f"{tag}: centre_track", cen.cpu(), r["centre"])


# ---- cvcl_maxpool3x3s2_idx ---------------------------------------------------------------------------------------------------------
def _run_maxpool_idx(dev, dt, shape, batch_chunk=None, torch_too=True):
    cd, tdt, epc = _dt(dt)
    lib = H.lib()
    B, Hh, W, C = shape
    Ho, Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    x = T.int_activations(shape, Hh * 31 + W + C, dev, lim=2).to(tdt)
    dy = T.int_activations((B, Ho, Wo, C), Hh * 7 + W, dev, lim=8).to(tdt)
    ybuf, y, ny = _out((B, Ho, Wo, C), tdt, dev, C)
    ibuf = torch.full((ny + 64,), CANARY8, dtype=torch.uint8, device=dev)
    idx = ibuf[:ny].view(B, Ho, Wo, C)
    dbuf, dx, nx = _out(shape, tdt, dev, C)
    H.check(lib.cvcl_maxpool3x3s2_idx(cd, H.ptr(x), None, H.ptr(y), H.ptr(idx), B, Hh, W, C, H.stream_ptr()), "maxpool_idx forward")
    H.check(lib.cvcl_maxpool3x3s2_idx(cd, None, H.ptr(dy), H.ptr(dx), H.ptr(idx), B, Hh, W, C, H.stream_ptr()), "maxpool_idx backward")
    torch.cuda.synchronize()
    pf, pb = T.flat_plan(ny // epc), T.flat_plan(nx // epc)
    step = batch_chunk or B
    for b0 in range(0, B, step):                          # (the float64 reference of the large cases in slices of the batch)
        b1 = min(B, b0 + step)
        tag = f"maxpool_idx {dt} {shape} images {b0}..{b1}"
        pooled, code = T.maxpool_idx_reference(x[b0:b1])
        _check(f"{tag}: pooled (b, oy, ox, c)", y[b0:b1], pooled, tdt, epc, pf["stride"], offset=b0 * Ho * Wo * C)
        bad = (idx[b0:b1] != code).nonzero()
        assert not len(bad), (f"{tag}: {len(bad)} arg-max bytes wrong; first at (b, oy, ox, c) = {bad[0].tolist()}: got "
                              f"{int(idx[b0:b1][tuple(bad[0].tolist())])}, want {int(code[tuple(bad[0].tolist())])}")
        _check(f"{tag}: dx (b, y, x, c)", dx[b0:b1], T.maxpool_bwd_reference(code, dy[b0:b1], Hh, W), tdt, epc, pb["stride"],
               offset=b0 * Hh * W * C)
        if torch_too:                                    # torch's own arg-max, on the CPU
            _v, ind = F.max_pool2d(x[b0:b1].double().cpu().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
            assert torch.equal(idx[b0:b1].cpu(), T.torch_codes(ind, W)), tag
    assert _tail_intact(ybuf, ny) and _tail_intact(dbuf, nx) and bool((ibuf[ny:] == CANARY8).all())
    return T.trips(ny // epc, pf), T.trips(nx // epc, pb)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", T.MAXPOOL_IDX_SHAPES, ids=["x".join(map(str, s)) for s in T.MAXPOOL_IDX_SHAPES])
def test_maxpool_idx_exact(dev, dt, shape):
    """inputs in {-2..2}, so nearly every window has several maxima: the pooled values, the recorded arg-max bytes (the FIRST maximum
    in row-major window order, as torch's return_indices) and the backward from them, dY in {-8..8}.  Even and odd extents, one-row
    and one-pixel maps."""
    assert _run_maxpool_idx(dev, dt, shape) == (1, 1)


def test_maxpool_idx_forward_past_the_grid_cap(dev):
    """fp32, 129 x 64 x 64 x 64: 2 113 536 output chunks on the 8192 x 256 threads the grid is capped at"""
    assert _run_maxpool_idx(dev, "f32", T.MAXPOOL_FWD_PAST_CAP, batch_chunk=16, torch_too=False)[0] == 2


def test_maxpool_idx_backward_past_the_grid_cap(dev):
    """fp32, 33 x 64 x 64 x 64: 2 162 688 input chunks on the capped grid"""
    assert _run_maxpool_idx(dev, "f32", T.MAXPOOL_BWD_PAST_CAP, batch_chunk=16, torch_too=False) == (1, 2)


# ---- cvcl_avgpool_bwd --------------------------------------------------------------------------------------------------------------
def _run_avgpool_bwd(dev, dt, B, HW, C):
    cd, tdt, _epc = _dt(dt)
    dp = T.int_activations((B, C), HW * 7 + C, dev, lim=64)
    buf, dx, n = _out((B, HW, C), tdt, dev, C)
    H.check(H.lib().cvcl_avgpool_bwd(cd, H.ptr(dp), H.ptr(dx), B, HW, C, H.stream_ptr()), "avgpool_bwd")
    torch.cuda.synchronize()
    q = T.avgpool_bwd_expected(dp, HW).to(dev)                              # the fp32 IEEE quotient, from the host
    exp = (q.to(BF) if tdt == BF else q)[:, None, :].expand(B, HW, C)
    p = T.flat_plan(n)
    wrong = _where(dx, exp.contiguous(), 1, p["stride"])
    assert not wrong, f"avgpool_bwd {dt} B={B} HW={HW} C={C}: (b, pixel, c) {wrong}"
    assert torch.equal(dx, exp) and _tail_intact(buf, n)
    return T.trips(n, p)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_avgpool_bwd_exact(dev, dt):
    """dx[b, p, c] = d_pooled[b, c] / HW: the correctly rounded fp32 quotient (then its bf16 rounding), for every pixel"""
    for HW in T.AVGPOOL_HW:
        for C in T.AVGPOOL_BWD_C:
            assert _run_avgpool_bwd(dev, dt, 3, HW, C) == 1


def test_avgpool_bwd_past_the_grid_cap(dev):
    assert _run_avgpool_bwd(dev, "f32", *T.AVGPOOL_BWD_PAST_CAP) == 2


# ---- cvcl_zero_stuff2 --------------------------------------------------------------------------------------------------------------
def _run_zero_stuff(dev, dt, shape):
    cd, tdt, epc = _dt(dt)
    B, Ho, Wo, C = shape
    dy = T.int_activations(shape, Ho * 5 + Wo + C, dev)
    dy = torch.where(dy == 0, torch.full_like(dy, 3.0), dy).to(tdt)          # no zeros: a stuffed zero is none of dy's
    buf, z, n = _out((B, 2 * Ho, 2 * Wo, C), tdt, dev, C)                     # (canary-filled: the zeros must be written)
    H.check(H.lib().cvcl_zero_stuff2(cd, H.ptr(dy), H.ptr(z), B, Ho, Wo, C, H.stream_ptr()), "zero_stuff2")
    torch.cuda.synchronize()
    p = T.flat_plan(n // epc)
    _check(f"zero_stuff2 {dt} {shape}: (b, y, x, c)", z, T.zero_stuff_reference(dy), tdt, epc, p["stride"])
    assert _tail_intact(buf, n)
    return T.trips(n // epc, p)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_zero_stuff2_exact(dev, dt):
    """z[b, 2 oy, 2 ox] = dy[b, oy, ox], zeros written everywhere else: one pixel of one chunk, odd extents, 3 (fp32: 6) chunks per
    pixel, and the layer-4 width"""
    for shape in T.ZERO_STUFF_SHAPES[dt]:
        assert _run_zero_stuff(dev, dt, shape) == 1


def test_zero_stuff2_past_the_grid_cap(dev):
    assert _run_zero_stuff(dev, "f32", T.ZERO_STUFF_PAST_CAP) == 2


# ---- cvcl_add, cvcl_relu_mask ------------------------------------------------------------------------------------------------------
def _run_add(dev, dt, chunks, relu):
    cd, tdt, epc = _dt(dt)
    n = chunks * epc
    a, b = T.int_activations((n,), chunks, dev).to(tdt), T.int_activations((n,), chunks + 1, dev).to(tdt)
    buf, y, _n = _out((n,), tdt, dev, 64)
    H.check(H.lib().cvcl_add(cd, H.ptr(a), H.ptr(b), H.ptr(y), n, relu, H.stream_ptr()), "add")
    torch.cuda.synchronize()
    ref = a.double() + b.double()
    assert bool((ref < 0).any()) or chunks == 1
    p = T.flat_plan(n)
    _check(f"add {dt} chunks={chunks} relu={relu}", y, torch.relu(ref) if relu else ref, tdt, epc, p["stride"])
    assert _tail_intact(buf, n)
    return T.trips(chunks, p)


def _run_relu_mask(dev, dt, chunks):
    cd, tdt, epc = _dt(dt)
    n = chunks * epc
    g = torch.Generator(device=dev).manual_seed(chunks)
    y = torch.tensor([0.0, -0.0, -1.0, -3.0, 0.5, 2.0], device=dev)[torch.randint(0, 6, (n,), generator=g, device=dev)]
    y[:6] = torch.tensor([0.0, -0.0, -1.0, 0.5, -0.0, 0.0][:min(n, 6)], device=dev)[:6]
    dy = T.int_activations((n,), chunks + 2, dev)
    dy = torch.where(dy == 0, torch.full_like(dy, -5.0), dy)                 # no zeros: a wrongly passed gradient shows
    buf, dx, _n = _out((n,), tdt, dev, 64)
    yt, gt = y.to(tdt), dy.to(tdt)
    H.check(H.lib().cvcl_relu_mask(cd, H.ptr(yt), H.ptr(gt), H.ptr(dx), n, H.stream_ptr()), "relu_mask")
    torch.cuda.synchronize()
    p = T.flat_plan(n)
    _check(f"relu_mask {dt} chunks={chunks}", dx, torch.where(y.double() > 0, dy.double(), 0.0), tdt, epc, p["stride"])
    assert _tail_intact(buf, n)
    return T.trips(chunks, p)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_add_and_relu_mask_exact(dev, dt):
    """y = a + b (ReLU or not) and dx = dy where y > 0, y of +0, -0, negatives and positives: one chunk, three, and 257 (a second
    workgroup)"""
    for chunks in T.FLAT_CHUNKS:
        assert _run_add(dev, dt, chunks, 0) == 1 and _run_add(dev, dt, chunks, 1) == 1
        assert _run_relu_mask(dev, dt, chunks) == 1


def test_add_and_relu_mask_past_the_grid_cap(dev):
    """fp32, 2 097 452 chunks: the last 300 are second trips of the grid-stride loop"""
    assert _run_add(dev, "f32", T.FLAT_PAST_CAP_CHUNKS, 1) == 2
    assert _run_relu_mask(dev, "f32", T.FLAT_PAST_CAP_CHUNKS) == 2


# ---- cvcl_gconv_weight_dgrad, cvcl_transpose ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,cg", T.WEIGHT_DGRAD_CASES)
def test_gconv_weight_dgrad_is_the_index_formula(dev, C, cg):
    """w = arange: out[g cg + ci][co_l][ky][kx] = w[g cg + co_l][ci][2 - ky][2 - kx], every element its own value"""
    n = C * cg * 9
    assert n < 2 ** 24
    w = torch.arange(n, dtype=F32, device=dev).view(C, cg, 3, 3)
    buf, out, _n = _out((C, cg, 3, 3), F32, dev, 64)
    H.check(H.lib().cvcl_gconv_weight_dgrad(H.ptr(w), H.ptr(out), C, cg, H.stream_ptr()), "gconv_weight_dgrad")
    torch.cuda.synchronize()
    _check(f"gconv_weight_dgrad C={C} cg={cg}: (o, col, ky, kx)", out, T.weight_dgrad_reference(w.double(), C, cg), F32, 1,
           T.flat_plan(n)["stride"])
    assert _tail_intact(buf, n)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", T.TRANSPOSE_CASES)
def test_transpose_moves_every_bit_pattern(dev, dt, rows, cols):
    """random finite bit patterns, compared as integers: one element, one row, partial 32 x 32 tiles in both directions, full
    tiles, and more than 64 tile rows"""
    cd, tdt, _epc = _dt(dt)
    bits = T.finite_bits((rows, cols), dt, rows * 3 + cols, dev)
    buf, out, n = _out((cols, rows), tdt, dev, 64)
    H.check(H.lib().cvcl_transpose(cd, H.ptr(bits.view(tdt)), H.ptr(out), rows, cols, H.stream_ptr()), "transpose")
    torch.cuda.synchronize()
    got = out.view(bits.dtype)
    bad = (got != bits.t()).nonzero()
    assert not len(bad), (f"transpose {dt} {rows} x {cols}: {len(bad)} wrong; first at out (c, r) = {bad[0].tolist()}, tile "
                          f"(bx, by) = ({int(bad[0][0]) // 32}, {int(bad[0][1]) // 32})")
    assert _tail_intact(buf, n)


# ---- cvcl_conv_wgrad_direct --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", T.WGRAD_CASES, ids=_ids(T.WGRAD_CASES))
def test_conv_wgrad_direct_exact(dev, dt, c):
    """operands in {-2..2}: every sum is an exact integer.  Grouped 3 x 3 at stride 1 and 2 on even, odd and non-square maps, two
    groups with twice as many outputs as inputs (the group formula), a 1 x 1 at stride 2, and the 7 x 7 / 2 stem on its NCHW fp32
    image with dY in either dtype"""
    cd, tdt, _epc = _dt(dt)
    Ho, Wo = T.conv_out(c["H"], c["k"], c["stride"], c["pad"]), T.conv_out(c["W"], c["k"], c["stride"], c["pad"])
    x = T.int_activations((c["B"], c["H"], c["W"], c["Cin"]), len(c["tag"]), dev, lim=2)
    dy = T.int_activations((c["B"], Ho, Wo, c["Cout"]), len(c["tag"]) + 1, dev, lim=2).to(tdt)
    xin = x.permute(0, 3, 1, 2).contiguous() if c["nchw"] else x.to(tdt)
    shape = (c["Cout"], c["cg"], c["k"], c["k"])
    buf, dw, n = _out(shape, F32, dev, 64)
    H.check(H.lib().cvcl_conv_wgrad_direct(cd, H.ptr(xin), H.ptr(dy), H.ptr(dw), c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["cg"],
                                           c["k"], c["stride"], c["pad"], 1 if c["nchw"] else 0, H.stream_ptr()), "conv_wgrad_direct")
    torch.cuda.synchronize()
    ref = T.conv_wgrad_reference(x, dy, c["cg"], c["k"], c["stride"], c["pad"])
    assert float(ref.abs().max()) > 0
    w = _first_wrong(dw, _expected(ref, F32))
    if w is not None:
        co, ci, ky, kx = w[1]
        raise AssertionError(f"conv_wgrad_direct {dt} {c['tag']}: (co, ci, ky, kx) {w[2]}; workgroup "
                             f"{((co * c['cg'] + ci) * c['k'] + ky) * c['k'] + kx}")
    assert torch.equal(dw, ref.float()) and _tail_intact(buf, n)


# ---- refusals of the chunk multiples -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_broken_chunks_are_refused(dev, dt):
    """n or C that is no multiple of the 16-byte chunk, and cvcl_bn_apply at 3 chunks per row: CVCL_EINVAL, every output at its canary"""
    cd, tdt, epc = _dt(dt)
    lib, s = H.lib(), H.stream_ptr()
    half = epc // 2
    a = torch.ones(64 * epc, dtype=tdt, device=dev)
    v = torch.ones(64 * epc, device=dev)
    buf, y, _n = _out((64 * epc,), tdt, dev, 0)
    ibuf = torch.full((64 * epc,), CANARY8, dtype=torch.uint8, device=dev)
    calls = [
        ("cvcl_add", lambda: lib.cvcl_add(cd, H.ptr(a), H.ptr(a), H.ptr(y), epc + half, 0, s)),
        ("cvcl_relu_mask", lambda: lib.cvcl_relu_mask(cd, H.ptr(a), H.ptr(a), H.ptr(y), epc + half, s)),
        ("cvcl_zero_stuff2", lambda: lib.cvcl_zero_stuff2(cd, H.ptr(a), H.ptr(y), 1, 1, 1, epc + half, s)),
        ("cvcl_maxpool3x3s2_idx", lambda: lib.cvcl_maxpool3x3s2_idx(cd, H.ptr(a), None, H.ptr(y), H.ptr(ibuf), 1, 2, 2, epc + half, s)),
        ("cvcl_maxpool3x3s2_idx", lambda: lib.cvcl_maxpool3x3s2_idx(cd, None, H.ptr(a), H.ptr(y), H.ptr(ibuf), 1, 2, 2, epc + half, s)),
        ("cvcl_bn_apply", lambda: lib.cvcl_bn_apply(cd, H.ptr(a), H.ptr(v), H.ptr(v), H.ptr(y), 2, epc + half, 1, s)),
        ("cvcl_bn_apply", lambda: lib.cvcl_bn_apply(cd, H.ptr(a), H.ptr(v), H.ptr(v), H.ptr(y), 2, 3 * epc, 1, s)),
    ]
    assert not T.bn_apply_supported(3 * epc, epc)
    for name, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == H.EINVAL and name in lib.cvcl_last_error().decode(), (name, rc)
        assert _untouched(buf) and bool((ibuf == CANARY8).all()), name
