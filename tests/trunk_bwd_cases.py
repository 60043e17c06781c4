"""The case tables of the trunk's backward-side kernels (csrc/trunk_bwd.hip: bn_apply, the three passes of bn_bwd, bn_moments, the
max pool with recorded arg-max in both directions, avgpool_bwd, zero_stuff, add, relu_mask, gconv_wflip, transpose,
conv_wgrad_direct), float64 references of each entry, operands on which every fp32 product, sum and fmaf is exact in any order, and
Python restatements of the launchers (chunk_grid, bn_bwd_rows and the cvcl_grid call sites).

As in stem_cases.py the restatements compute no expected value: they let a case assert that it runs in the regime it was chosen for
(row lanes without a row, a partial group of the 4-row unroll, several trips of the row loop, a capped or rounded grid, a second
grid-stride trip).  If a launcher changes in the library, the assertion fails and says so; the case is then chosen anew.

BatchNorm backward operands (bn_bwd_inputs): x, dy small integers, mean a small integer, rstd and gamma powers of two, so that
xhat = (x - mean) * rstd, every product g * xhat and every sub-sum of them is a small multiple of a power of two; where the row count
n is a power of two as well, 1 / n, the three coefficients and both fused multiply-adds of dx are exact (bn_bwd_exactness proves it
case by case).  Every 16-byte channel chunk has its own constants, so a thread that used another chunk's vectors is caught."""
import torch
import torch.nn.functional as F

from stem_cases import AFFINE_ROWS, AVGPOOL_HW, MAXPOOL_SHAPES, cvcl_grid, div_up, int_activations, pool_affine  # noqa: F401

F64 = torch.float64
BF = torch.bfloat16
U = 2.0 ** -24                                  # unit roundoff of fp32
U16 = 2.0 ** -8                                 # unit roundoff of bf16 (8 significand bits)
GRID_CAP = 8192                                 # the cap of the cvcl_grid(.., 256, 8192) call sites
CHUNK_GRID_CAP = 16384                          # the cap inside chunk_grid


def epc_of(dt):
    """restates epc_of: elements of a 16-byte chunk"""
    return 8 if dt == "bf16" else 4


# ---- the launchers, restated ------------------------------------------------------------------------------------------------------
def chunk_grid(total_chunks, cc, per_thread):
    """restates chunk_grid: the capped grid, rounded up so that grid * 256 is a multiple of the cc chunks of a row"""
    mult = 1
    while (mult * 256) % cc:
        mult += 1
    g = max(1, min(div_up(total_chunks, 256 * per_thread), CHUNK_GRID_CAP))
    return div_up(g, mult) * mult


def bn_apply_supported(C, epc):
    """restates the argument checks of cvcl_bn_apply"""
    if C <= 0 or C % epc:
        return False
    cc = C // epc
    return cc & (cc - 1) == 0 or 256 % cc == 0 or cc % 256 == 0


def bn_apply_plan(rows, C, epc):
    """restates cvcl_bn_apply and the walk of bn_apply_kernel: thread i0 takes the chunks i0, i0 + stride, .."""
    cc = C // epc
    total = rows * cc
    capped = max(1, min(div_up(total, 1024), CHUNK_GRID_CAP))
    grid = chunk_grid(total, cc, 4)
    return dict(cc=cc, total=total, capped=capped, grid=grid, rounded=grid != capped, stride=grid * 256,
                trips=div_up(total, grid * 256), fixed_chunk=(grid * 256) % cc == 0)


def bn_bwd_supported(C, epc):
    """restates the channel check of cvcl_bn_bwd: C / chunk a power of two"""
    return C > 0 and C % epc == 0 and (C // epc) & (C // epc - 1) == 0


def bn_bwd_rows(epc, rows, C):
    """restates bn_bwd_rows (what cvcl_bn_bwd_partial_rows returns): the x extent of the reduce pass's grid"""
    cc = C // epc
    ccb = min(cc, 256)
    rl, ny = 256 // ccb, cc // ccb
    cap = max(512 // ny, 1)
    return max(1, min(div_up(rows, rl * 8), cap))


def bn_bwd_plan(epc, rows, C):
    """restates cvcl_bn_bwd: the reduce grid (g, ny) of ccb chunk columns x RL row lanes per workgroup, the row walk of
    bn_bwd_reduce_kernel (row r = bx * RL + lane + k * g * RL, four k per trip), the partial rows one slice of the finalize pass
    reads, and the apply pass's grid (two chunks i, i + stride per trip)"""
    cc = C // epc
    ccb = min(cc, 256)
    RL, ny = 256 // ccb, cc // ccb
    g = bn_bwd_rows(epc, rows, C)
    rstep = g * RL
    total = rows * cc
    agrid = chunk_grid(total, cc, 4)
    return dict(cc=cc, ccb=ccb, RL=RL, ny=ny, g=g, cap=max(512 // ny, 1), capped=g == max(512 // ny, 1) and div_up(rows, RL * 8) > g,
                rstep=rstep, trips=div_up(rows, 4 * rstep), idle_lanes=max(0, rstep - rows), partial_unroll=rows % (4 * rstep) != 0,
                rows_per_lane=div_up(rows, rstep), finalize_reads=div_up(g, 64), agrid=agrid, astride=agrid * 256, total=total,
                atrips=div_up(total, 2 * agrid * 256))


def bn_bwd_block_of_row(rows, p):
    """[rows] long: the partial row (blockIdx.x of bn_bwd_reduce_kernel) that adds input row r"""
    return (torch.arange(rows) % p["rstep"]) // p["RL"]


def flat_plan(units):
    """restates the cvcl_grid(units, 256, 8192) call sites: cvcl_add and cvcl_relu_mask (units = n ELEMENTS, the kernel then walks
    n / chunk chunks), cvcl_maxpool3x3s2_idx, cvcl_zero_stuff2, cvcl_gconv_weight_dgrad (units = chunks or weights) and
    cvcl_avgpool_bwd (units = elements)"""
    grid = cvcl_grid(units, 256, GRID_CAP)
    return dict(grid=grid, stride=grid * 256)


def trips(work, p):
    """grid-stride trips the busiest thread makes over ``work`` items on the grid of plan ``p``"""
    return div_up(work, p["stride"])


# ---- float64 references -----------------------------------------------------------------------------------------------------------
def bn_apply_reference(x, scale, shift, relu):
    y = x.to(F64) * scale.to(F64) + shift.to(F64)
    return torch.relu(y) if relu else y


def bn_bwd_reference(mode, x, out, dy, scale, shift, mean, rstd, gamma):
    """cvcl_bn_bwd's contract in float64, nothing rounded: x, dy (and out for mode 2) [rows, C]; the per-channel vectors [C].
    g = dy * mask (mode 0: none; 1: x * scale + shift > 0; 2: out > 0), dbeta = sum g, dgamma = sum g * xhat with
    xhat = (x - mean) * rstd, and dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n) in the kernel's form k1 g + (k2 x + k3).
    Also returned: the inner fma k2 x + k3 and the four terms whose magnitudes carry the rounding bound of the ragged cases."""
    x64, dy64 = x.to(F64), dy.to(F64)
    mean64, rstd64, gamma64 = mean.to(F64), rstd.to(F64), gamma.to(F64)
    n = torch.full_like(mean64, float(x.shape[0]))          # (a tensor: a true division on any device)
    if mode == 0:
        g = dy64
    elif mode == 1:
        g = torch.where(x64 * scale.to(F64) + shift.to(F64) > 0, dy64, torch.zeros_like(dy64))
    else:
        g = torch.where(out.to(F64) > 0, dy64, torch.zeros_like(dy64))
    xhat = (x64 - mean64) * rstd64
    dbeta, dgamma = g.sum(dim=0), (g * xhat).sum(dim=0)
    k1 = gamma64 * rstd64
    k2 = -k1 * rstd64 * dgamma / n
    a0 = -k1 * dbeta / n
    k3 = a0 - k2 * mean64
    inner = k2 * x64 + k3
    return dict(g=g, dbeta=dbeta, dgamma=dgamma, k1=k1, k2=k2, k3=k3, a0=a0, k2mean=k2 * mean64, inner=inner, dx=k1 * g + inner,
                magnitude=(k1 * g).abs() + (k2 * x64).abs() + a0.abs() + (k2 * mean64).abs())


def bn_moments_reference(stats, count, eps, centre):
    """bn_moments_kernel's contract in float64 on the kernel's fp32 inputs: mean = sum / count, biased variance clamped at 0,
    rstd = 1 / sqrt(var + (double)(float)eps), centre + mean.  On the CPU (IEEE division and square root)."""
    s = stats.to(F64).cpu().sum(dim=0)
    cnt = torch.full_like(s[0], float(count))
    mean = s[0] / cnt
    raw_var = s[1] / cnt - mean * mean
    var = torch.clamp(raw_var, min=0.0)
    e = float(torch.tensor(eps, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + e)
    return dict(mean=mean, raw_var=raw_var, var=var, rstd=rstd, centre=None if centre is None else centre.to(F64).cpu() + mean,
                unbiased_rstd=1.0 / torch.sqrt(var * count / max(count - 1, 1) + e))


def maxpool_idx_reference(x):
    """cvcl_maxpool3x3s2_idx forward in float64: x [B, H, W, C] -> (pooled [B, Ho, Wo, C], code [B, Ho, Wo, C] uint8): 3 x 3 maximum,
    stride 2, pad 1, and the window position ky * 3 + kx of the FIRST maximum in row-major order (a later tap replaces the maximum
    only where it is greater).  Nine tap-shifted views of the -inf padded map."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x.to(F64), (0, 0, 1, 1, 1, 1), value=float("-inf"))
    m = torch.full((B, Ho, Wo, C), float("-inf"), dtype=F64, device=x.device)
    k = torch.zeros((B, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
            better = v > m
            m = torch.where(better, v, m)
            k = torch.where(better, torch.full_like(k, ky * 3 + kx), k)
    return m, k


def maxpool_bwd_reference(code, dy, H, W):
    """the backward from the recorded codes in float64: dx [B, H, W, C], dx[b, 2 oy - 1 + ky, 2 ox - 1 + kx] += dy[b, oy, ox] where
    code == ky * 3 + kx"""
    B, Ho, Wo, C = dy.shape
    dxp = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=F64, device=dy.device)       # padded by one pixel in front
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2] += torch.where(code == ky * 3 + kx, dy.to(F64), 0.0)
    return dxp[:, 1:1 + H, 1:1 + W].contiguous()


def torch_codes(indices, W):
    """torch's max_pool2d(3, 2, 1, return_indices=True) indices [B, C, Ho, Wo] (flat positions iy * W + ix of the input plane) ->
    the window codes ky * 3 + kx [B, Ho, Wo, C] uint8"""
    _B, _C, Ho, Wo = indices.shape
    iy, ix = indices // W, indices % W
    oy = torch.arange(Ho, device=indices.device).view(1, 1, Ho, 1)
    ox = torch.arange(Wo, device=indices.device).view(1, 1, 1, Wo)
    code = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    return code.permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def avgpool_bwd_expected(dp, HW):
    """[B, C] fp32 -> the fp32 IEEE quotient dp / (float)HW, computed on the host"""
    d = dp.float().cpu()
    return d / torch.full_like(d, float(HW))


def zero_stuff_reference(dy):
    B, Ho, Wo, C = dy.shape
    z = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=F64, device=dy.device)
    z[:, ::2, ::2] = dy.to(F64)
    return z


def weight_dgrad_reference(w, C, cg):
    """cvcl_gconv_weight_dgrad by its index formula: w [C, cg, 3, 3] (OIHW) -> out[g cg + ci][co_l][ky][kx] =
    w[g cg + co_l][ci][2 - ky][2 - kx]"""
    G = C // cg
    return w.reshape(G, cg, cg, 9).permute(0, 2, 1, 3).flip(-1).reshape(C, cg, 3, 3).contiguous()


def conv_wgrad_reference(x_nhwc, dy, cg, k, stride, pad):
    """cvcl_conv_wgrad_direct's contract in float64: x [B, H, W, Cin], dy [B, Ho, Wo, Cout] -> dW [Cout, cg, k, k],
    dW[co][ci][ky][kx] = sum_{b, oy, ox} dy[b, oy, ox, co] x[b, oy s - pad + ky, ox s - pad + kx, group(co) cg + ci], with
    group(co) = co / (Cout / groups) and groups = Cin / cg.  k x k tap-shifted views (no library convolution)."""
    B, H, W, Cin = x_nhwc.shape
    _B, Ho, Wo, Cout = dy.shape
    G = Cin // cg
    xp = F.pad(x_nhwc.to(F64), (0, 0, pad, pad, pad, pad)).view(B, H + 2 * pad, W + 2 * pad, G, cg)
    d = dy.to(F64).view(B, Ho, Wo, G, Cout // G)
    dw = torch.zeros(G, Cout // G, cg, k, k, dtype=F64, device=dy.device)
    for ky in range(k):
        for kx in range(k):
            xt = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            dw[:, :, :, ky, kx] = torch.einsum("bhwgo,bhwgi->goi", d, xt)
    return dw.view(Cout, cg, k, k)


def conv_out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def bn_bwd_inputs(rows, C, seed, device, lim=None):
    """Operands of one cvcl_bn_bwd shape for all three modes, fp32 tensors whose values bf16 holds too.
    x, dy [rows, C]: integers within +-lim (4 up to 1024 rows, 2 beyond: dx stays within 24 bits as the sums grow).
    mean: integers in -3..3; rstd in {1/4, 1/2, 1, 2}; gamma in +-{1/2, 1, 2, 4}; no two channel chunks of 4 share their constants.
    mode 1: the forward's own affine scale = gamma rstd, shift = beta - mean scale with beta = scale b0, b0 an integer in -2..2, so
    that the pre-activation scale (x - mean + b0) is exactly 0 wherever x = mean - b0.
    mode 2: out in {+0, -0, 1/2, 1, 3}."""
    g = torch.Generator(device=device).manual_seed(seed)
    if lim is None:
        lim = 4 if rows <= 1024 else 2
    x, dy = _ints(g, (rows, C), -lim, lim, device), _ints(g, (rows, C), -lim, lim, device)
    c = torch.arange(C, device=device)
    mean = ((c * 5 + c // 7 + seed) % 7 - 3).float()
    rstd = torch.tensor([1.0, 0.5, 2.0, 0.25], device=device)[(c + c // 4 + c // 28) % 4]
    gamma = torch.tensor([1.0, -0.5, 2.0, 4.0, -1.0, 0.5, -2.0, -4.0], device=device)[(c * 3 + c // 8 + c // 112) % 8]
    b0 = ((c * 2 + c // 5) % 5 - 2).float()
    scale = gamma * rstd
    shift = scale * (b0 - mean)
    out = torch.tensor([0.0, -0.0, 0.5, 1.0, 3.0], device=device)[torch.randint(0, 5, (rows, C), generator=g, device=device)]
    return dict(x=x, dy=dy, out=out, mean=mean, rstd=rstd, gamma=gamma, scale=scale, shift=shift, b0=b0, lim=lim)


def chunk_constants_differ(t, epc=4):
    """no two 16-byte channel chunks share (mean, rstd, gamma, scale, shift)"""
    v = torch.stack([t[k].double().cpu() for k in ("mean", "rstd", "gamma", "scale", "shift")], dim=1)       # [C, 5]
    rows = [tuple(r) for r in v.view(-1, epc * 5).tolist()]
    return len(set(rows)) == len(rows)


def is_f32(v):
    """the float64 tensor is representable in fp32"""
    return bool(torch.equal(v.float().double(), v))


def bn_bwd_exactness(t, r, p):
    """t: bn_bwd_inputs, r: bn_bwd_reference of one mode, p: bn_bwd_plan.  -> list of what is NOT exact for the kernel (empty: the
    case is exact).  The kernel holds in fp32: the partial sums of g and g * xhat of each (workgroup, channel) -- every sub-sum, in
    any order, is exact where the sum of magnitudes stays below 2^24 units of the channel's quantum (1 for g, rstd for g xhat);
    dbeta and dgamma; 1 / n; k1, k2, k3 and the product k2 * mean inside k3; the inner and the outer fma of dx."""
    bad = []
    rows = t["x"].shape[0]
    if rows & (rows - 1):
        bad.append("rows is no power of two: 1 / n is rounded")
    blk = bn_bwd_block_of_row(rows, p).to(r["g"].device)
    z = torch.zeros(p["g"], r["g"].shape[1], dtype=F64, device=r["g"].device)
    xhat_units = (t["x"].double() - t["mean"].double())                       # xhat in units of rstd: an integer
    if float(z.index_add(0, blk, r["g"].abs()).max()) >= 2 ** 24:
        bad.append("a workgroup's sum of |g| reaches 2^24")
    if float(z.index_add(0, blk, (r["g"] * xhat_units).abs()).max()) >= 2 ** 24:
        bad.append("a workgroup's sum of |g xhat| reaches 2^24 quanta")
    for k in ("dbeta", "dgamma", "k1", "k2", "k3", "k2mean", "a0", "inner", "dx"):
        if not is_f32(r[k]):
            bad.append(f"{k} is not representable in fp32")
    if float(r["g"].abs().sum(dim=0).max()) >= 2 ** 24 or float((r["g"] * xhat_units).abs().sum(dim=0).max()) >= 2 ** 24:
        bad.append("a channel's sum of magnitudes reaches 2^24: dbeta / dgamma may be rounded")
    return bad


def bn_bwd_partials(r, t, p):
    """the partial rows [g, 2, C] float64 the reduce pass must write (exact where bn_bwd_exactness is empty)"""
    rows = t["x"].shape[0]
    blk = bn_bwd_block_of_row(rows, p).to(r["g"].device)
    z = torch.zeros(p["g"], r["g"].shape[1], dtype=F64, device=r["g"].device)
    xhat = (t["x"].double() - t["mean"].double()) * t["rstd"].double()
    return torch.stack([z.index_add(0, blk, r["g"]), z.index_add(0, blk, r["g"] * xhat)], dim=1)


def moments_inputs(rows, C, count, seed, device, negative_var=False):
    """statistics rows [rows, 2, C] whose float64 column sums are exactly count * mean and count * (var + mean^2), mean a multiple of
    1/4 within +-8 and var in {0, 0.75, 3.75, 15.75}; a centre of halves.  (stem_cases.finalize_exact_inputs)"""
    from stem_cases import finalize_exact_inputs
    t = finalize_exact_inputs(rows, C, count, seed, device, centre=True, negative_var=negative_var)
    return dict(stats=t["stats"], mean=t["mean"], var=t["var"], centre=t["centre"])


def finite_bits(shape, dt, seed, device):
    """random bit patterns of finite values (an all-ones exponent gets its lowest bit cleared) -> int32 (fp32) or int16 (bf16)"""
    g = torch.Generator(device=device).manual_seed(seed)
    if dt == "bf16":
        b = torch.randint(0, 1 << 16, shape, generator=g, device=device, dtype=torch.int32)
        b = torch.where((b & 0x7F80) == 0x7F80, b & ~0x0080, b)
        return (b - ((b & 0x8000) << 1)).to(torch.int16)
    b = torch.randint(0, 1 << 32, shape, generator=g, device=device, dtype=torch.int64)
    b = torch.where((b & 0x7F800000) == 0x7F800000, b & ~0x00800000, b)
    return (b - ((b & 0x80000000) << 1)).to(torch.int32)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
def case(tag, dt, C, rows, **claims):
    return dict(tag=tag, dt=dt, C=C, rows=rows, **claims)


# cvcl_bn_bwd, exact: rows a power of two
BN_BWD_EXACT = [
    case("bf16_C8_rows1", "bf16", 8, 1, RL=256, g=1, idle_lanes=255, trips=1),
    case("bf16_C8_rows64", "bf16", 8, 64, RL=256, g=1, idle_lanes=192, trips=1),
    case("bf16_C8_rows4096", "bf16", 8, 4096, RL=256, g=2, idle_lanes=0, trips=2),
    case("bf16_C64_rows64", "bf16", 64, 64, RL=32, g=1, rows_per_lane=2, partial_unroll=True, trips=1),
    case("bf16_C64_rows1024", "bf16", 64, 1024, RL=32, g=4, trips=2),
    case("bf16_C2048_rows8192", "bf16", 2048, 8192, RL=1, ny=1, g=512, capped=True, trips=4, finalize_reads=8),
    case("f32_C4_rows2", "f32", 4, 2, RL=256, g=1, idle_lanes=254, trips=1),
    case("f32_C256_rows1024", "f32", 256, 1024, RL=4, g=32, trips=2),
    case("f32_C2048_rows4096", "f32", 2048, 4096, RL=1, ny=2, g=256, cap=256, capped=True, trips=4),
]
BN_BWD_CLAIMS = ("RL", "ny", "g", "cap", "capped", "idle_lanes", "trips", "rows_per_lane", "partial_unroll", "finalize_reads")

# cvcl_bn_bwd, ragged: the row counts of stem_cases.AFFINE_ROWS beyond 1, and one past a power of two
BN_BWD_RAGGED_ROWS = [3, 98, 1000, 1100, 4097]


def bn_bwd_ragged_channels(dt):
    return [epc_of(dt), 64, 256, 2048]


# cvcl_bn_batch_moments
MOMENTS_ROWS = [1, 3, 8, 9, 513]
MOMENTS_C = [4, 32, 100, 2048]
MOMENTS_COUNT = 4096                            # a power of two
MOMENTS_RAGGED_COUNT = 12544                    # 112 x 112: no power of two

# cvcl_bn_apply: chunks per row; 768 makes the launcher round its grid to a multiple of 3
BN_APPLY_CC = [1, 8, 256, 768]
BN_APPLY_PAST_CAP = (21846, 6144)               # bf16 (rows, C): 16 777 728 chunks

# cvcl_maxpool3x3s2_idx: the maps of stem_cases.MAXPOOL_SHAPES (and a single pixel), at C = 8
MAXPOOL_IDX_SHAPES = sorted({(B, H, W, 8) for B, H, W, _C in MAXPOOL_SHAPES} | {(1, 1, 1, 8)})
MAXPOOL_FWD_PAST_CAP = (129, 64, 64, 64)        # fp32: 129 * 32 * 32 * 16 = 2 113 536 output chunks
MAXPOOL_BWD_PAST_CAP = (33, 64, 64, 64)         # fp32: 33 * 64 * 64 * 16 = 2 162 688 input chunks

AVGPOOL_BWD_C = [8, 100, 2048]
AVGPOOL_BWD_PAST_CAP = (65, 16, 2048)           # (B, HW, C): 2 129 920 elements

ZERO_STUFF_SHAPES = dict(bf16=[(1, 1, 1, 8), (2, 3, 5, 64), (3, 4, 4, 24), (2, 7, 7, 2048)],
                         f32=[(1, 1, 1, 4), (2, 3, 5, 64), (3, 4, 4, 24), (2, 7, 7, 2048)])            # (B, Ho, Wo, C)
ZERO_STUFF_PAST_CAP = (33, 32, 32, 64)          # fp32: 33 * 64 * 64 * 16 = 2 162 688 chunks

FLAT_CHUNKS = [1, 3, 257]                       # cvcl_add, cvcl_relu_mask: n in chunks
FLAT_PAST_CAP_CHUNKS = GRID_CAP * 256 + 300     # fp32: 2 097 452 chunks, 33.6 MB

WEIGHT_DGRAD_CASES = [(32, 1), (64, 2), (128, 4), (1024, 32), (2048, 64)]                                # (C, cin_per_group)

TRANSPOSE_CASES = [(1, 1), (1, 40), (33, 31), (64, 64), (100, 2048), (2050, 130)]                       # (rows, cols)


def wcase(tag, B, H, W, Cin, Cout, cg, k, stride, pad, nchw=False):
    return dict(tag=tag, B=B, H=H, W=W, Cin=Cin, Cout=Cout, cg=cg, k=k, stride=stride, pad=pad, nchw=nchw)


WGRAD_CASES = [
    wcase("g3x3_2x8x8_C128_s1", 2, 8, 8, 128, 128, 4, 3, 1, 1),
    wcase("g3x3_2x8x8_C128_s2", 2, 8, 8, 128, 128, 4, 3, 2, 1),
    wcase("g3x3_1x7x7_C64_s2", 1, 7, 7, 64, 64, 2, 3, 2, 1),
    wcase("g3x3_2x6x6_C32_s1", 2, 6, 6, 32, 32, 1, 3, 1, 1),
    wcase("g3x3_2x5x9_C64_s2", 2, 5, 9, 64, 64, 2, 3, 2, 1),
    wcase("two_groups_8_to_16", 2, 6, 6, 8, 16, 4, 3, 1, 1),
    wcase("c1x1_s2_16_to_32", 2, 7, 7, 16, 32, 16, 1, 2, 0),
    wcase("stem_2x3x18x22", 2, 18, 22, 3, 64, 3, 7, 2, 3, nchw=True),
]
