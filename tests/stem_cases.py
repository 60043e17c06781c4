"""The case tables of the ResNeXt forward kernels around the grouped convolution (csrc/stem.hip: the four stem kernels; csrc/bn.hip:
bn_finalize, bn_eval_affine, col_stats, bn_relu_maxpool, bn_add_relu, bn_relu_apply, avgpool), exact float64 references of each
entry, operands on which every fp32 product, sum, fmaf and maximum is exact in any order, and Python restatements of the launchers.

The restatements compute no expected value: they let a case assert that it runs in the regime it was chosen for (which fp32 stem
kernel, a shrunk band, a second grid-stride trip, the XCD-major item order, a grid that had to be rounded).  If a launcher changes
in the library, the assertion fails and says so; the case is then chosen anew.

Stem operands: x in {-4..4}, w in {-2..2}, centres multiples of 0.5.  A uniformly random 147-tap sum has a standard deviation of
about 45, so it would never leave the range where bf16 holds every half exactly; each image therefore carries one 12 x 12 blob of
{2, 3, 4} and two output channels (ALIGNED: all taps +1, all taps -1) answer it with about +-440, where bf16 keeps even integers
only and every odd result is a tie.  Those two channels have integer centres, so that their squares are integers and a workgroup's
fp32 sum of them stays exact (stem_stats_bound)."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
BF = torch.bfloat16
STEM_TH = 4                                    # STEM_TH: output rows per work item of stem_mfma_kernel
STEMP_TP, STEMP_BW = 2, 128                    # STEMP_TP pooled rows per item, STEMP_BW band pixels of stem_pool_mfma_kernel
ALIGNED = (5, 40)                              # output channels with all-equal taps (+1, -1): one below 32, one above
BLOB = 12


def div_up(a, b):
    return -(-a // b)


def cvcl_grid(items, per_block, cap):
    """restates cvcl_grid (csrc/cvcl_common.h)"""
    return max(1, min(div_up(items, per_block), cap))


# ---- the launchers, restated ------------------------------------------------------------------------------------------------------
def bf16_stem_supported(H, W):
    """restates the argument checks of the bf16 branch of cvcl_stem_conv7x7 (STEM_PITCH = 144)"""
    return H % 2 == 0 and W % 2 == 0 and W + 6 + 8 <= 2 * 144 and W % 4 == 0 and W // 4 <= 64


def bf16_stem_plan(B, H, W):
    """restates stem_grid, and the band / m-tile / item walk of stem_mfma_kernel"""
    Ho, Wo = H // 2, W // 2
    bands = div_up(Ho, STEM_TH)
    items = B * bands
    grid = min(items, 512)
    return dict(Ho=Ho, Wo=Wo, TH=STEM_TH, bands=bands, items=items, grid=grid, trips=div_up(items, grid), xcd=grid % 8 == 0,
                mtiles=div_up(Wo, 16), partial_band=Ho % STEM_TH != 0, partial_tile=Wo % 16 != 0, supported=bf16_stem_supported(H, W))


def first_item(block, grid):
    """restates ``bx`` of stem_mfma_kernel / stem_pool_mfma_kernel: the first work item of workgroup ``block`` (XCD-major where the
    grid is a multiple of 8, plain otherwise); its later items are first_item + k * grid"""
    return (block & 7) * (grid >> 3) + (block >> 3) if grid % 8 == 0 else block


def item_workgroup(item, grid):
    """the ``bx`` that runs ``item``: item % grid, in the plain and in the XCD-major order alike (a grid-stride loop from bx)"""
    return item % grid


def f32_stem_plan(B, H, W):
    """restates the fp32 branch of cvcl_stem_conv7x7: ``lds_of``, the TH choice, tiled or direct, and the grid"""
    Ho, Wo = H // 2, W // 2

    def lds_of(th):
        return (147 * 64 + 64 + 3 * (2 * th + 5) * (W + 6)) * 4
    TH = min(Ho, 8)
    while TH > 1 and lds_of(TH) > 150 * 1024:
        TH -= 1
    tiled = lds_of(TH) <= 150 * 1024
    if not tiled:
        return dict(Ho=Ho, Wo=Wo, tiled=False, TH=1, bands=Ho, items=B * Ho, grid=cvcl_grid(B * Ho * Wo * 64, 256, 8192),
                    partial_band=False, lds=0)
    bands = div_up(Ho, TH)
    items = B * bands
    return dict(Ho=Ho, Wo=Wo, tiled=True, TH=TH, bands=bands, items=items, grid=min(items, 1024), partial_band=Ho % TH != 0,
                lds=lds_of(TH), trips=div_up(items, min(items, 1024)))


def stem_pool_supported(H, W):
    """restates cvcl_stem_pool_supported for bf16"""
    return H % 2 == 0 and W % 4 == 0 and W // 4 <= 64 and W + 6 + 8 <= 2 * 144 and W // 2 + 2 <= STEMP_BW


def stem_pool_plan(B, H, W, cus):
    """restates cvcl_stem_pool and the item walk of stem_pool_mfma_kernel; ``cus`` is the device's compute-unit count"""
    Ho, Wo = H // 2, W // 2
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    bands = div_up(Hp, STEMP_TP)
    items = B * bands
    grid = min(items, cus)
    mtiles = div_up(Wo, 16)
    return dict(Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp, TH=STEMP_TP, bands=bands, items=items, grid=grid, trips=div_up(items, grid),
                xcd=grid % 8 == 0, mtiles=mtiles, partial_band=Hp % STEMP_TP != 0,
                # the last m-tile's lane 15 stores at band column mtiles * 16: the column behind the band row where that is STEMP_BW
                tile_past_row=mtiles * 16 + 1 > STEMP_BW, supported=stem_pool_supported(H, W))


def maxpool_plan(B, H, W, C):
    """restates the grid of cvcl_bn_relu_maxpool (POOL_ROWS = 2 output rows per thread, 8 channels per thread)"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    total = B * div_up(Ho, 2) * Wo * (C // 8)
    grid = cvcl_grid(total, 256, 8192)
    return dict(Ho=Ho, Wo=Wo, total=total, grid=grid, trips=div_up(total, grid * 256))


def affine_plan(rows, C, epc):
    """restates the grid of cvcl_bn_add_relu / cvcl_bn_relu_apply: a multiple of cc / gcd(cc, 256), so that grid * 256 chunks is
    a multiple of the cc = C / epc chunks of a row and a thread keeps its channel chunk; epc = 8 (bf16) or 4 (fp32)"""
    cc = C // epc
    mult = cc // math.gcd(cc, 256)
    capped = cvcl_grid(rows * cc, 256 * 4, 16384)
    grid = div_up(capped, mult) * mult
    stride, total = grid * 256, rows * cc
    return dict(cc=cc, mult=mult, capped=capped, grid=grid, stride=stride, total=total, rounded=grid != capped,
                trips=div_up(total, 2 * stride), several=total > stride,
                # in the last trip some thread has a first chunk i < total whose second chunk i + stride is not (has_j == false):
                # whenever that trip is not a full one; and where more than a stride is left of it, other threads have both
                tail=total % (2 * stride) != 0, tail_both=total % (2 * stride) > stride)


def avgpool_plan(B, C):
    """restates the grid of cvcl_avgpool"""
    grid = cvcl_grid(B * C, 256, 4096)
    return dict(grid=grid, trips=div_up(B * C, grid * 256))


def col_stats_rows(rows):
    """restates cvcl_col_stats_rows"""
    return min(max(div_up(rows, 256), 1), 256)


def col_stats_block(rows, g):
    """[rows] long: the partial row (blockIdx.x of col_stats_kernel) that adds input row r: r = block * 4 + slice + k * g * 4"""
    return (torch.arange(rows) // 4) % g


# ---- float64 references -----------------------------------------------------------------------------------------------------------
def stem_reference(x, w, centre):
    """cvcl_stem_conv7x7's contract in float64: x [B, 3, H, W] (NCHW), w [64, 3, 7, 7] (OIHW), centre [64] or None ->
    [B, H/2, W/2, 64] (NHWC): 7 x 7 convolution, stride 2, zero padding 3, minus centre.  49 tap-shifted views times the [3 -> 64]
    weight slice of the tap (no library convolution)."""
    B, _, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = F.pad(x.to(F64), (3, 3, 3, 3))
    w64 = w.to(F64)
    out = torch.zeros(B, Ho, Wo, 64, dtype=F64, device=x.device)
    for ky in range(7):
        for kx in range(7):
            xt = xp[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
            out += torch.einsum("bchw,oc->bhwo", xt, w64[:, :, ky, kx])
    if centre is not None:
        out = out - centre.to(F64)
    return out


def maxpool_reference(x, scale, shift):
    """cvcl_bn_relu_maxpool's contract in float64: x [B, H, W, C] -> [B, Ho, Wo, C]: 3 x 3 maximum, stride 2, pad 1, over
    relu(x * scale + shift).  Nine tap-shifted views of the zero-padded activation (zero = the ReLU's floor)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    act = torch.relu(x.to(F64) * scale.to(F64) + shift.to(F64))
    ap = F.pad(act, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, Ho, Wo, C, dtype=F64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, ap[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2])
    return out


def stem_pool_reference(x, w, centre, scale, shift):
    """cvcl_stem_pool's contract: maxpool(relu(bf16(conv - centre) * scale + shift)) in float64 (its bf16 rounding is the output)"""
    raw = stem_reference(x, w, centre).float().to(BF)
    return maxpool_reference(raw, scale, shift)


def bn_add_relu_reference(raw, scale, shift, idn, idn_scale, idn_shift):
    v = raw.to(F64) * scale.to(F64) + shift.to(F64)
    r = idn.to(F64) if idn_scale is None else idn.to(F64) * idn_scale.to(F64) + idn_shift.to(F64)
    return torch.relu(v + r)


def bn_finalize_reference(stats, count, gamma, beta, rm, rv, momentum, eps, centre):
    """bn_finalize_kernel's contract in float64 on the kernel's fp32 inputs, nothing rounded: stats [rows, 2, C] fp32 partial sums
    -> dict of float64 [C]: mean, var (E[x^2] - mean^2 clamped at 0), scale = gamma / sqrt(var + eps), shift = beta - mean * scale,
    true_mean = mean + centre, unbiased = var * count / (count - 1) (var itself for count == 1: evaluated as the kernel does, left
    to right), and the two running statistics m * new + (1 - m) * old; m, eps and 1 - m are the fp32 values the kernel sees.
    ``running_var_2`` is the same with the new value rounded to fp32 first, as the kernel hands it to its fused multiply-add:
    where everything else is exact, the kernel's running_var is that value's fp32 rounding."""
    f32 = torch.float32
    s = stats.to(F64).sum(dim=0)
    # (divisors as tensors of the operand's shape: on a GPU torch divides by a Python scalar by multiplying with its reciprocal,
    # which is no correctly rounded division)
    cnt, cnt_1 = torch.full_like(s[0], float(count)), torch.full_like(s[0], float(count - 1))
    mean = s[0] / cnt
    var = torch.clamp(s[1] / cnt - mean * mean, min=0.0)
    m, e = float(torch.tensor(momentum, dtype=f32)), float(torch.tensor(eps, dtype=f32))
    one_m = float(torch.tensor(1.0, dtype=f32) - torch.tensor(momentum, dtype=f32))
    scale = gamma.to(F64) / torch.sqrt(var + e)
    unbiased = (var * cnt) / cnt_1 if count > 1 else var
    true_mean = (mean + centre.to(F64)) if centre is not None else mean
    return dict(mean=mean, var=var, scale=scale, shift=beta.to(F64) - mean * scale, true_mean=true_mean, unbiased=unbiased, m=m,
                one_m=one_m, running_mean=m * true_mean + one_m * rm.to(F64), running_var=m * unbiased + one_m * rv.to(F64),
                running_var_2=m * unbiased.float().to(F64) + one_m * rv.to(F64))


def bn_eval_affine_reference(gamma, beta, rm, rv, eps, centre):
    """bn_eval_affine_kernel's contract in float64: scale = gamma / sqrt(rv + eps), shift = beta - (rm - centre) * scale"""
    e = float(torch.tensor(eps, dtype=torch.float32))
    scale = gamma.to(F64) / torch.sqrt(rv.to(F64) + e)
    d = rm.to(F64) - centre.to(F64) if centre is not None else rm.to(F64)
    return dict(scale=scale, d=d, shift=beta.to(F64) - d * scale)


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def stem_inputs(B, H, W, seed, centre=True):
    """x [B, 3, H, W] in {-4..4} with one BLOB x BLOB patch of {2, 3, 4} per image, w [64, 3, 7, 7] in {-2..2} with the two
    ALIGNED channels all +1 / all -1, centre [64]: non-zero multiples of 0.5 within +-8 (integers in the ALIGNED channels), or
    None.  |y| <= 147 * 4 * 2 + 8 = 1184: in units of 0.5 far below 2^24, every fp32 partial sum is exact in any order.  (CPU)"""
    g = torch.Generator().manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    x = ints((B, 3, H, W), -4, 4)
    bh, bw = min(BLOB, H), min(BLOB, W)
    y0 = torch.randint(0, H - bh + 1, (B,), generator=g).tolist()
    x0 = torch.randint(0, W - bw + 1, (B,), generator=g).tolist()
    for b in range(B):
        x[b, :, y0[b]:y0[b] + bh, x0[b]:x0[b] + bw] = ints((3, bh, bw), 2, 4)
    w = ints((64, 3, 7, 7), -2, 2)
    w[ALIGNED[0]] = 1.0
    w[ALIGNED[1]] = -1.0
    cen = None
    if centre:
        cen = ints((64,), 1, 16) * 0.5 * (ints((64,), 0, 1) * 2 - 1)
        for ch in ALIGNED:
            cen[ch] = torch.sign(cen[ch]) * torch.ceil(cen[ch].abs())   # (a half -> the next integer away from 0)
        assert bool((cen != 0).all()) and float(cen.abs().max()) <= 8 and torch.equal(cen * 2, (cen * 2).round())
    assert float(x.abs().max()) <= 4 and float(w.abs().max()) <= 2
    return x, w, cen


def pool_affine(C, seed=0):
    """scale [C]: powers of two 1/4 .. 4; shift [C]: multiples of 1/8 in [-32, 32).  (scale, shift) differs in every channel for
    C <= 2560: the shift walks all 512 values (37 is odd) and the scale, which changes from channel to channel, takes another of its
    five values each time the shift comes round again.  Half the shifts are negative: negative pre-activations.  (CPU)"""
    c = torch.arange(C)
    shift = (((c * 37 + 11 * seed) % 512) - 256).float() / 8
    scale = torch.tensor([1.0, 0.5, 2.0, 0.25, 4.0])[((c % 512) + 2 * (c // 512) + seed) % 5]
    assert C > 2560 or len({(float(a), float(b)) for a, b in zip(scale, shift)}) == C
    return scale, shift


def int_activations(shape, seed, device, lim=32):
    """integers in [-lim, lim] as fp32 (exact in bf16 up to 256)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g, device=device).float()


# ---- exactness bounds -------------------------------------------------------------------------------------------------------------
def wg_partials(v, TH, bands, grid):
    """v [B, Ho, Wo, C] float64, non-negative -> [C]: the largest sum any workgroup accumulates.  Work item (b, band) = b * bands +
    band goes to the workgroup whose bx is item % grid (item_workgroup)."""
    B, Ho, Wo, C = v.shape
    per_item = F.pad(v, (0, 0, 0, 0, 0, bands * TH - Ho)).view(B * bands, TH * Wo, C).sum(dim=1)
    trips = div_up(per_item.shape[0], grid)
    per_wg = F.pad(per_item, (0, 0, 0, trips * grid - per_item.shape[0])).view(trips, grid, C).sum(dim=0)
    return per_wg.max(dim=0).values


def quantum(e):
    """e [.., C] float64 -> [C]: 0.25 where a channel holds an odd multiple of 0.5 (its squares are multiples of 0.25), else 1"""
    flat = e.reshape(-1, e.shape[-1])
    assert torch.equal(flat * 2, (flat * 2).round())
    return torch.where(((flat * 2) % 2 != 0).any(dim=0), 0.25, 1.0).to(F64)


def stem_stats_bound(exp, p):
    """exp [B, Ho, Wo, 64]: the expected bf16 output (any float dtype).  -> (largest workgroup sum of |y| in units of 0.5, largest
    workgroup sum of y^2 in units of the channel's quantum): both below 2^24 means every fp32 sub-sum a workgroup forms, in any
    order, is exact."""
    e = exp.to(F64)
    return (float((wg_partials(e.abs(), p["TH"], p["bands"], p["grid"]) * 2).max()),
            float((wg_partials(e * e, p["TH"], p["bands"], p["grid"]) / quantum(e)).max()))


def col_stats_bound(y, g):
    """y [rows, C] -> the same two figures for the partial rows of col_stats_kernel on a grid of g"""
    e = y.to(F64)
    blk = col_stats_block(e.shape[0], g).to(e.device)
    z = torch.zeros(g, e.shape[1], dtype=F64, device=e.device)
    return (float((z.index_add(0, blk, e.abs()) * 2).max()), float((z.index_add(0, blk, e * e) / quantum(e)).max()))


# ---- case tables ------------------------------------------------------------------------------------------------------------------
def case(tag, B, H, W, **claims):
    return dict(tag=tag, B=B, H=H, W=W, **claims)


# cvcl_stem_conv7x7, bf16 (stem_mfma_kernel)
BF16_STEM_CASES = [
    case("one_band_1x8x64", 1, 8, 64, bands=1, items=1),
    case("partial_band_and_tile_2x36x72", 2, 36, 72, partial_band=True, partial_tile=True),
    case("tall_1x64x32", 1, 64, 32),
    case("widest_1x32x256", 1, 32, 256, mtiles=8),
    case("narrow_3x32x16", 3, 32, 16, mtiles=1, partial_tile=True),                # Wo = 8 < 16: one m-tile per row, 4 waves
    case("second_trip_65x64x64", 65, 64, 64, items=520, grid=512, xcd=True, trips=2),
    case("plain_order_5x24x64", 5, 24, 64, items=15, grid=15, xcd=False, trips=1),
]
BF16_STEM_REFUSALS = [case("W260", 1, 8, 260), case("W66", 1, 8, 66), case("H9", 1, 9, 64)]

# cvcl_stem_conv7x7, fp32 (stem_tiled_f32_kernel, stem_direct_f32_kernel)
F32_STEM_CASES = [
    case("tiled_TH8_2x64x64", 2, 64, 64, tiled=True, TH=8),
    case("tiled_partial_1x36x72", 1, 36, 72, tiled=True, TH=8, partial_band=True),
    case("tiled_TH7_1x20x456", 1, 20, 456, tiled=True, TH=7, partial_band=True),
    case("tiled_TH1_1x6x1370", 1, 6, 1370, tiled=True, TH=1),
    case("tiled_second_trip_129x128x32", 129, 128, 32, tiled=True, TH=8, items=1032, grid=1024, trips=2),
    case("direct_1x4x1372", 1, 4, 1372, tiled=False),
    case("direct_2x6x1376", 2, 6, 1376, tiled=False),
]

# cvcl_stem_pool (stem_pool_mfma_kernel).  ``cus``: the compute-unit count the claim about the grid holds for (an MI355X has 256)
STEM_POOL_CASES = [
    case("W224_2x16x224", 2, 16, 224, mtiles=7, tile_past_row=False),
    case("W228_2x16x228", 2, 16, 228, mtiles=8, tile_past_row=True),
    case("W240_2x16x240", 2, 16, 240, mtiles=8, tile_past_row=True),
    case("W252_2x16x252", 2, 16, 252, mtiles=8, tile_past_row=True),
    case("partial_band_2x36x72", 2, 36, 72, Hp=9, partial_band=True),
    case("small_1x8x16", 1, 8, 16, items=1),
    case("second_trip_65x32x228", 65, 32, 228, items=260, trips=2, cus=256, tile_past_row=True),
    # (a workgroup reads -centre anew for every tile but writes it once, before its first item: what the last tile of an item
    # overwrites is wrong for the workgroup's NEXT item, so the widths above need a second trip each to show it)
    case("second_trip_129x16x240", 129, 16, 240, items=258, trips=2, cus=256, tile_past_row=True),
    case("second_trip_129x16x252", 129, 16, 252, items=258, trips=2, cus=256, tile_past_row=True),
    case("plain_order_3x24x64", 3, 24, 64, items=9, xcd=False),
]

# cvcl_bn_relu_maxpool: (B, H, W, C); the first eight are the shapes of test_resnext_gpu.test_bn_relu_maxpool_shapes
MAXPOOL_SHAPES = [(2, 16, 16, 64), (1, 15, 17, 64), (3, 14, 9, 64), (1, 7, 7, 64), (2, 113, 112, 64), (2, 112, 112, 64),
                  (1, 1, 5, 64), (1, 2, 2, 64), (2, 9, 7, 8), (2, 9, 7, 72)]
MAXPOOL_PAST_CAP = (65, 64, 64, 512)

# cvcl_bn_add_relu / cvcl_bn_relu_apply
# 1100 rows: at 3, 5 or 9 (fp32: 6, 10, 18) chunks per row the capped grid (4, 6, 10; 7, 11, 20) is no multiple of 3, 5, 9 and is
# rounded, AND every thread takes several chunks -- the one size here at which a thread relies on the rounding
AFFINE_ROWS = [1, 3, 98, 1000, 1100]


def affine_channels(epc):
    return [epc, 24, 40, 72, 256, 2048]


AFFINE_PAST_CAP = dict(f32=(2796300, 24), bf16=(5592500, 24))                       # (rows, C): rows * C / epc just above 16384 x 1024

AVGPOOL_HW = [1, 7, 8, 9, 49, 64]
AVGPOOL_C = [8, 100, 2048]
AVGPOOL_PAST_CAP = (520, 1, 2048)                                                   # (B, HW, C)

COL_STATS_ROWS = [1, 3, 5, 1024, 65536 + 7]
COL_STATS_C = [8, 64, 100, 192]

FINALIZE_ROWS = [1, 63, 64, 65, 512, 513, 1025]
FINALIZE_C = [1, 15, 16, 17, 64, 2048]
FINALIZE_COUNTS = [1, 2, 12544]


def finalize_exact_inputs(rows, C, count, seed, device, centre=True, negative_var=False):
    """Hand-made partial rows stats [rows, 2, C] whose float64 column sums are EXACTLY count * mean and count * (var + mean^2) for a
    per-channel mean (a multiple of 1/4 within +-8) and a var in {0, 0.75, 3.75, 15.75}: with eps = 0.25, var + eps is a power of
    four, its root a power of two, and with dyadic gamma / beta / running statistics and momentum 0.5 every operation of
    bn_finalize_kernel is exact.  negative_var: the sum of squares is count * (mean^2 - 2^-6), E[x^2] - mean^2 = -2^-6 < 0, which
    must clamp to var = 0.  All partial values are multiples of 2^-6 below 2^17 or of 1/4 below 2^21: exact in fp32, their sums exact in float64."""
    g = torch.Generator(device=device).manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device=device).to(F64)
    mean = ints((C,), -32, 32) / 4
    var = torch.tensor([0.0, 0.75, 3.75, 15.75], dtype=F64, device=device)[ints((C,), 0, 3).long()]
    second = mean * mean + var
    if negative_var:
        var = torch.zeros_like(var)
        second = mean * mean - 2.0 ** -6
    tot = torch.stack([mean * count, second * count])                               # [2, C]
    parts = ints((rows, 2, C), -64, 64) / 4                                          # arbitrary rows ...
    parts[rows - 1] = 0
    parts[rows - 1] = tot - parts.sum(dim=0)                                         # ... and the one that makes the sums come out
    stats = parts.float()
    assert torch.equal(stats.to(F64), parts) and torch.equal(stats.to(F64).sum(dim=0), tot)
    gamma = torch.tensor([0.5, 1.0, -2.0, 4.0], device=device)[ints((C,), 0, 3).long()]
    beta = (ints((C,), -16, 16) / 4).float()
    rm, rv = (ints((C,), -16, 16) / 4).float(), (ints((C,), 0, 32) / 4).float()
    cen = (ints((C,), -16, 16) / 2).float() if centre else None
    return dict(stats=stats, mean=mean, var=var, gamma=gamma, beta=beta, rm=rm, rv=rv, centre=cen, eps=0.25, momentum=0.5)
