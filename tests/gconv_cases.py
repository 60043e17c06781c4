"""The case tables of cvcl_gconv3x3 (csrc/gconv.hip: gconv_mfma_kernel<WIDE, NPF, NMT> for bf16, gconv_tiled_f32_kernel<CG> and
gconv_direct_f32_kernel for fp32), an exact float64 reference of the entry, integer-valued operands on which every fp32 sum is
exact in any order, and Python restatements of the two launch plans.

The plans compute no expected value: they let a case assert that it runs in the regime it was chosen for (several work items per
workgroup, the XCD-major item order, a partial last band, a given kernel instantiation).  If a plan changes in the library, the
assertion fails and says so; the case is then chosen anew.

A case is a dict: tag, C, H, W, stride, B and, for bf16, what it claims: ``inst`` (WIDE, NPF, NMT), ``grid``, ``items`` and the
regime flags ``multi`` (grid < items), ``xcd`` (grid % 8 == 0 with several trips), ``partial`` (Ho % TH != 0).  groups is 32
everywhere (the trunk's cardinality), so C = 128 .. 1024 gives 4 .. 32 channels per group; WIDE means 32 of them."""
import torch
import torch.nn.functional as F

GROUPS = 32
PIXB = 144                                     # GC_PIXB: LDS bytes per staged pixel
F64 = torch.float64


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ---- the launch plans, restated ---------------------------------------------------------------------------------------------------
def bf16_plan(B, H, W, C, stride):
    """restates gconv_plan and the instantiation choice of cvcl_gconv3x3_src (csrc/gconv.hip)"""
    Ho, Wo = out_hw(H, W, stride)
    Wp = W + 2

    def rows_in(th):
        return (th - 1) * stride + 3

    def lds(th):
        return (rows_in(th) * Wp + th * Wo) * PIXB
    TH = Ho
    while TH > 1 and (lds(TH) > 52 * 1024 or rows_in(TH) * Wp > 10 * 32 or TH * Wo > 128):
        TH = (TH + 1) // 2
    cg = C // GROUPS
    bands = -(-Ho // TH)
    per_cu = max(1, min(160 * 1024 // lds(TH), 2 if cg == 32 else 3))
    items = B * bands
    grid_x = min(items, max(1, per_cu * 256 // max(C // 64, 1)))
    staged = rows_in(TH) * Wp
    slots = -(-staged // 32)
    bucket = 4 if slots <= 4 else 6 if slots <= 6 else 8 if slots <= 8 else 10
    few = TH * Wo <= 64
    supported = (C % GROUPS == 0 and cg in (4, 8, 16, 32) and C % 64 == 0 and lds(TH) <= 160 * 1024 and staged <= 10 * 32 and
                 TH * Wo <= 128)
    return dict(TH=TH, bands=bands, rows_in=rows_in(TH), grid_x=grid_x, items=items, slots=bucket, few=few, supported=supported,
                staged=staged, lds=lds(TH), inst=(cg == 32, bucket, 4 if few else 8), partial=Ho % TH != 0,
                trips=-(-items // grid_x))


def f32_plan(B, H, W, C, stride, aligned=True):
    """restates the fp32 branch of cvcl_gconv3x3_src (csrc/gconv.hip): the tiled kernel's band rule and grid, or the direct kernel"""
    Ho, Wo = out_hw(H, W, stride)
    cg = C // GROUPS

    def plane_p(th):
        pl = ((th - 1) * stride + 3) * (W + 2)
        return pl + ((9 - (pl & 7)) & 7)

    def lds(th):
        return (64 * 9 * cg + 64 + 64 * plane_p(th)) * 4
    TH = Ho
    while TH > 1 and lds(TH) > 150 * 1024:
        TH -= 1
    tiled = C % 64 == 0 and cg in (4, 8, 16, 32) and lds(TH) <= 150 * 1024 and aligned
    bands = -(-Ho // TH)
    items = B * bands
    gx = min(max(1024 // max(C // 64, 1), 1), items)
    return dict(tiled=tiled, TH=TH, bands=bands, items=items, gx=gx, partial=Ho % TH != 0, cg=cg,
                last_n_out=(Ho - (bands - 1) * TH) * Wo, n_out=min(TH, Ho) * Wo)


# ---- the float64 reference --------------------------------------------------------------------------------------------------------
def gconv_reference(x, scale, shift, w, centre, stride, groups):
    """cvcl_gconv3x3's contract in float64: x [B, H, W, C] (NHWC), w [C, C / groups, 3, 3] (OIHW), scale / shift / centre [C] or None
    -> [B, Ho, Wo, C].  Activation relu(x * scale + shift) (x itself without a prologue), zero padding AFTER it, grouped 3 x 3
    convolution with pad 1, minus centre.  Nine tap-shifted views times the per-group weight blocks (no library convolution: on the
    GPU those are not exact on integers)."""
    B, H, W, C = x.shape
    cg = C // groups
    Ho, Wo = out_hw(H, W, stride)
    act = x.to(F64)
    if scale is not None:
        act = torch.relu(act * scale.to(F64) + shift.to(F64))
    xp = F.pad(act, (0, 0, 1, 1, 1, 1))
    wg = w.to(F64).view(groups, cg, cg, 3, 3)                                        # [group][co][ci][ky][kx]
    out = torch.zeros(B * Ho * Wo, groups, cg, dtype=F64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            xt = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(-1, groups, cg)
            out += torch.einsum("mgi,goi->mgo", xt, wg[:, :, :, ky, kx])
    out = out.view(B, Ho, Wo, C)
    if centre is not None:
        out = out - centre.to(F64)
    return out


# ---- integer-valued operands ------------------------------------------------------------------------------------------------------
def gconv_inputs(case, seed, device="cpu", prologue=True, centre=True, B=None):
    """x, w in {-2..2}, scale in {0.5, 1, 2}, shift in {-2..2} (every third channel in {1, 2}: there relu(shift) > 0, and a padding
    pixel staged as relu(shift) instead of 0 is a wrong border value), centre in {-8..8}.  The activation is a multiple of 0.5 of at
    most 6 (exact in bf16), every product a multiple of 0.5 of at most 12, every partial sum a multiple of 0.5 below 2^23: exact in
    fp32 in any order.  -> dict(x [B,H,W,C] f32, w [C,cg,3,3] f32, scale, shift, centre ([C] f32 or None), bound)"""
    Bn = case["B"] if B is None else B
    C, H, W = case["C"], case["H"], case["W"]
    cg = C // GROUPS
    g = torch.Generator(device=device).manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()
    x = ints((Bn, H, W, C), -2, 2)
    w = ints((C, cg, 3, 3), -2, 2)
    scale = shift = cen = None
    act_max = 2.0
    if prologue:
        scale = torch.tensor([0.5, 1.0, 2.0], device=device)[torch.randint(0, 3, (C,), generator=g, device=device)]
        shift = ints((C,), -2, 2)
        shift[::3] = ints((len(shift[::3]),), 1, 2)
        assert int((shift > 0).sum()) * 3 >= C
        assert set(scale.unique().tolist()) <= {0.5, 1.0, 2.0}
        act = torch.relu(x * scale + shift)
        assert torch.equal(act * 2, (act * 2).round()) and torch.equal(act.bfloat16().float(), act)       # a multiple of 0.5, exact in bf16
        act_max = 6.0
        assert float(act.max()) <= act_max
    if centre:
        cen = ints((C,), -8, 8)
    assert float(x.abs().max()) <= 2 and float(w.abs().max()) <= 2
    bound = 9 * cg * act_max * 2 + (8 if centre else 0)                 # |y|: 9 taps x cg channels x |act| x |w| + |centre|
    assert bound <= 3464 and bound * 2 < 2 ** 24                        # in units of 0.5 still below 2^24: exact in fp32
    return dict(x=x, w=w, scale=scale, shift=shift, centre=cen, bound=bound)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
def case(tag, C, H, W, stride, B, inst=None, **claims):
    return dict(tag=tag, C=C, H=H, W=W, stride=stride, B=B, inst=inst, **claims)


N_, W_ = False, True                                                    # narrow (4 / 8 / 16 channels per group), wide (32)

# bf16, several work items per workgroup on the trunk's own geometries
TRUNK_CASES = [
    case("l1_56_s1_B14", 128, 56, 56, 1, 14, (N_, 8, 8), grid=384, items=392, multi=True, xcd=True),
    case("l2_56_s2_B14", 256, 56, 56, 2, 14, (N_, 10, 4), grid=192, items=196, multi=True, xcd=True),
    case("l2_28_s1_B28", 256, 28, 28, 1, 28, (N_, 6, 8), grid=192, items=196, multi=True, xcd=True),
    case("l3_28_s2_B25", 512, 28, 28, 2, 25, (N_, 10, 4), grid=96, items=100, multi=True, xcd=True, partial=True),
    case("l3_14_s1_B49", 512, 14, 14, 1, 49, (N_, 6, 8), grid=96, items=98, multi=True, xcd=True),
    case("l4_14_s2_B33", 1024, 14, 14, 2, 33, (W_, 8, 4), grid=32, items=33, multi=True, xcd=True),
    case("l4_7_s1_B33", 1024, 7, 7, 1, 33, (W_, 4, 4), grid=32, items=33, multi=True, xcd=True),
    case("wide_56_s1_B3", 1024, 56, 56, 1, 3, (W_, 8, 8), grid=32, items=84, multi=True, xcd=True, trips=3),
    case("l1_56_s1_B13", 128, 56, 56, 1, 13, (N_, 8, 8), grid=364, items=364, multi=False, xcd=False, trips=1),
]

# bf16, the remaining instantiations and edge geometry: B = 3, each narrow (C 128) and wide (C 1024)
_EDGE_GEOMETRY = [
    # (H, W, stride, (NPF, NMT) or None, claims)
    (9, 25, 2, (10, 8), {}),
    (5, 13, 1, (4, 8), {}),
    (1, 41, 1, (6, 4), {}),
    (1, 41, 2, (6, 4), {}),
    (1, 63, 1, (8, 4), {}),
    (1, 63, 2, (8, 4), dict(n_out=32)),                                 # exactly two full m-tiles
    (2, 33, 1, (6, 8), dict(n_out=66)),                                 # an odd count of m-tiles (5): the pair loop's lone tile
    (2, 47, 1, (8, 8), {}),
    (63, 2, 2, (10, 4), dict(TH=32)),                                   # the largest band-row index the tile table packs
    (1, 1, 1, None, dict(n_out=1)),
    (1, 1, 2, None, dict(n_out=1)),
    (25, 25, 2, None, dict(partial=True, odd_s2=True)),
    (13, 27, 1, None, dict(partial=True)),
    (30, 20, 2, None, dict(partial=True)),
    (20, 30, 1, None, dict(partial=True)),
    (3, 104, 2, None, dict(staged=318)),                                # the widest supported row: 3 x 106 of the 320 slots
    (104, 3, 1, None, {}),
]
EDGE_CASES = [case(f"{'wide' if wide else 'narrow'}_{H}x{W}_s{s}", 1024 if wide else 128, H, W, s, 3,
                   None if nn is None else (wide,) + nn, **cl)
              for (H, W, s, nn, cl) in _EDGE_GEOMETRY for wide in (N_, W_)]

BF16_CASES = TRUNK_CASES + EDGE_CASES
ALL_INSTANTIATIONS = {(wide, npf, nmt) for wide in (N_, W_) for npf in (4, 6, 8, 10) for nmt in (4, 8)}


def by_tag(tag):
    (c,) = [c for c in BF16_CASES + F32_CASES if c["tag"] == tag]
    return c


# the variations run on these three
VARIATION_TAGS = ["l2_56_s2_B14", "wide_56_s1_B3", "narrow_9x25_s2"]
ACCUMULATE_TAGS = ["l3_28_s2_B25", "l4_14_s2_B33"]

# (H, W, stride, C, text cvcl_last_error must contain)
REFUSALS = [
    dict(tag="row_321_pixels", C=128, H=3, W=105, stride=1, B=3, msg="too wide for one staged band"),
    dict(tag="C96", C=96, H=8, W=8, stride=1, B=3, msg="unsupported channels-per-group"),
    dict(tag="short_stats", C=128, H=56, W=56, stride=1, B=14, msg="stats_rows", rows_short=1),
]

# fp32.  Tiled kernel, one case per channels-per-group with more (image, band) items than workgroups (the item loop's second trip),
# on the trunk's geometries; then edge geometry.  ``second_trip`` / ``partial`` / ``ragged`` (n_out % 64 != 0: idle lanes in the last
# pixel block) are asserted from f32_plan.
F32_CASES = [
    case("f32_cg4_56_s1_B65", 128, 56, 56, 1, 65, second_trip=True),
    case("f32_cg8_28_s1_B129", 256, 28, 28, 1, 129, second_trip=True),
    case("f32_cg16_28_s2_B65", 512, 28, 28, 2, 65, second_trip=True),
    case("f32_cg16_14_s1_B129", 512, 14, 14, 1, 129, second_trip=True),
    case("f32_cg32_14_s2_B65", 1024, 14, 14, 2, 65, second_trip=True),
    case("f32_cg32_7_s1_B65", 1024, 7, 7, 1, 65, second_trip=True),
    case("f32_partial_58_s1", 128, 58, 58, 1, 2, partial=True, ragged=True),
    case("f32_25x25_s2", 256, 25, 25, 2, 3, ragged=True),
    case("f32_13x27_s1", 512, 13, 27, 1, 3, ragged=True),
    case("f32_1x1", 1024, 1, 1, 1, 3, ragged=True),
    case("f32_misaligned_x", 512, 14, 14, 1, 3, misaligned=True),
]
