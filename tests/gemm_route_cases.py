"""The case table of cvcl_gemm's routing (csrc/gemm.hip plan_gemm; DESIGN.md "GEMM routing"): every route and both sides of every
threshold at the smallest shapes that still select the route, the statistics forms, and every refusal of cvcl_gemm.

A case is a dict: tag, dt (_hip dtype), M, N, K and options (see build_args).  build_args turns one into a cvcl_gemm_args block with
pointers from ``alloc`` -- dummy aligned integers for the device-free probes, tensors on the GPU.  ``want`` names the route a case
is meant to exercise (documentation; the tests check what can be observed: row counts, outputs, messages); ``refuse`` is the
text cvcl_gemm must leave in cvcl_last_error.
"""
import ctypes as C

from multimodal import _hip as H

F32, BF16, F32X3 = H.F32, H.BF16, H.F32X3
NONE, RELU, GELU, QUICK = H.ACT_NONE, H.ACT_RELU, H.ACT_GELU, H.ACT_QUICK_GELU
DUMMY = 4096                                               # a non-null, 16-byte aligned stand-in pointer


def case(tag, dt, M, N, K, want, **opt):
    return dict(tag=tag, dt=dt, M=M, N=N, K=K, want=want, **opt)


LN_MSG = ("cvcl_gemm: ln_stats / row_part (LayerNorm folded into the linear) exist in the 8-wave bf16 kernel only; these arguments do "
          "not select it (M {M} N {N} K {K}) -- ask cvcl_gemm_ln_supported first")

CASES = [
    # ---- 8-wave kernel: 96 tiles of 256 rows, K >= 256, N K >= 170 (N + K)
    case("g8_conv_96tiles", BF16, 12288, 512, 512, "8w/0", stats="rows"),
    case("g8_conv_95tiles", BF16, 12032, 512, 512, "glds/0", stats="rows"),
    case("g8_conv_k128", BF16, 12288, 512, 128, "glds/0", stats="rows"),
    case("g8_conv_nk_above", BF16, 24576, 256, 512, "8w/0", stats="rows"),
    case("g8_conv_nk_below", BF16, 24576, 256, 384, "glds/0", stats="rows"),
    case("g8_conv_acc", BF16, 12288, 512, 512, "8w/0", stats="acc"),
    case("g8_conv_short", BF16, 12288, 512, 512, "8w/0 -> glds/0", stats="short"),
    case("g8_conv_centre", BF16, 12288, 512, 512, "8w/0", stats="rows", centre=True),
    case("g8_conv_statsonly", BF16, 12288, 512, 512, "8w/0", stats="rows", no_C=True),
    case("g8_conv_gather", BF16, 12544, 512, 512, "8w/0", stats="rows", gather=(7, 7, 14, 14, 2)),
    case("g8_plain_nostats", BF16, 12288, 512, 512, "8w/0 (entry: linear walk)"),
    case("g8_lin_bias", BF16, 12288, 512, 512, "8w/1", bias=True),
    case("g8_lin_gelu", BF16, 12288, 512, 512, "8w/1", bias=True, act=GELU),
    case("g8_lin_relu", BF16, 12288, 512, 512, "8w/1", bias=True, act=RELU),
    case("g8_lin_res", BF16, 12288, 512, 512, "8w/1", bias=True, residual=True),
    case("g8_lin_res_act", BF16, 12288, 512, 512, "glds/3", bias=True, residual=True, act=RELU),
    case("g8_lin_95tiles", BF16, 12032, 512, 512, "glds/4", bias=True, act=GELU),
    case("g8_ln_stats", BF16, 12288, 512, 512, "8w/1", bias=True, act=GELU, ln="consumer"),
    case("g8_row_part", BF16, 12288, 512, 512, "8w/1", bias=True, residual=True, ln="producer"),
    # ---- streaming kernel: plain operand from 2^17 rows, BN + ReLU operand at any M
    case("pro_plain_2p17", BF16, 131072, 256, 128, "pro", stats="rows"),
    case("pro_plain_below", BF16, 131071, 256, 128, "glds/0", stats="rows"),
    case("pro_plain_acc", BF16, 131072, 256, 128, "pro", stats="acc"),
    case("pro_plain_nostats", BF16, 131072, 256, 256, "pro"),
    case("pro_bn_small", BF16, 32768, 256, 128, "pro", stats="rows", prologue="bn_relu"),
    case("pro_bn_ragged", BF16, 32801, 256, 256, "pro", stats="rows", prologue="bn_relu"),
    case("pro_bn_statsonly", BF16, 32768, 256, 128, "pro", stats="rows", prologue="bn_relu", no_C=True),
    case("pro_bn_short", BF16, 32768, 256, 128, "pro -> tiled", stats="short", prologue="bn_relu"),
    case("pro_tail", BF16, 4096, 256, 128, "pro", prologue="bn_relu", tail=True, residual=True, act=RELU),
    case("pro_tail_rscale", BF16, 4096, 256, 128, "pro", prologue="bn_relu", tail=True, r_scale=True, residual=True, act=RELU),
    # ---- direct-to-LDS kernel, every EPI
    case("glds0_stats", BF16, 1000, 256, 64, "glds/0", stats="rows"),
    case("glds0_acc", BF16, 1000, 256, 64, "glds/0", stats="acc"),
    case("glds0_short", BF16, 1000, 256, 64, "glds/0", stats="short"),
    case("glds0_multiblock", BF16, 70000, 128, 64, "glds/0", stats="rows"),
    case("glds1_bias_res", BF16, 300, 128, 64, "glds/1", bias=True, residual=True),
    case("glds2_tail", BF16, 1000, 256, 64, "glds/2", tail=True, residual=True, act=RELU),
    case("glds2_tail_rscale", BF16, 1000, 256, 64, "glds/2", tail=True, r_scale=True, residual=True, act=RELU),
    case("glds3_relu", BF16, 300, 128, 64, "glds/3", bias=True, act=RELU),
    case("glds4_gelu", BF16, 300, 128, 64, "glds/4", bias=True, act=GELU),
    case("glds5_c_pre", BF16, 300, 128, 64, "glds/5", bias=True, act=GELU, C_pre=True),
    case("glds6_g", BF16, 300, 128, 64, "glds/6", G=True),
    # ---- tiled kernel: PRO 0 / 1 / 2, lean and not, both dtypes
    case("tiled_bf16_p0_lean", BF16, 300, 128, 96, "tiled/0/lean", stats="rows"),
    case("tiled_bf16_p0", BF16, 300, 120, 96, "tiled/0", bias=True),
    case("tiled_bf16_p1_lean", BF16, 300, 128, 64, "tiled/1/lean", prologue="bn", stats="rows"),
    case("tiled_bf16_p1", BF16, 300, 128, 64, "tiled/1", prologue="bn", bias=True),
    case("tiled_bf16_p2_lean", BF16, 300, 128, 64, "tiled/2/lean", prologue="bn_relu", stats="rows"),
    case("tiled_bf16_p2", BF16, 300, 128, 64, "tiled/2", prologue="bn_relu", residual=True),
    case("tiled_bf16_p2_short", BF16, 300, 128, 64, "tiled/2/lean", prologue="bn_relu", stats="short"),
    case("tiled_bf16_gather", BF16, 2 * 49, 128, 96, "tiled/0/lean", stats="rows", gather=(7, 7, 14, 14, 2)),
    case("tiled_f32_p0_lean", F32, 300, 128, 96, "tiled/0/lean", stats="rows"),
    case("tiled_f32_p0", F32, 300, 128, 96, "tiled/0", residual=True),
    case("tiled_f32_p1_lean", F32, 300, 128, 64, "tiled/1/lean", prologue="bn", stats="rows"),
    case("tiled_f32_p1", F32, 300, 128, 64, "tiled/1", prologue="bn", bias=True),
    case("tiled_f32_p2_lean", F32, 300, 128, 64, "tiled/2/lean", prologue="bn_relu", stats="rows"),
    case("tiled_f32_p2", F32, 300, 128, 64, "tiled/2", prologue="bn_relu", bias=True, act=GELU),
    case("tiled_f32_short", F32, 300, 128, 96, "tiled/0/lean", stats="short"),
    # ---- fp32 small kernel against the tiled one (t_small = M N K / 13.4e6 + 5 against 12 + 4.6 K / 64 per round of 256 tiles)
    case("f32_small_below", F32, 1152, 1152, 256, "small/0"),
    case("f32_small_above", F32, 1160, 1152, 256, "tiled/0/lean"),
    case("f32_small_bias_scale", F32, 33, 50, 64, "small/0", bias=True, exp_scale=True),
    # ---- fp32 split arithmetic: small against the 64 x 64 split kernel (6 + tiles K/32 / 1024 + K / 128), then the tiled TR 4-7
    case("f32_split_small", F32, 384, 384, 256, "small/0", split=True),
    case("f32_split_64", F32, 448, 448, 256, "split64/0", split=True),
    case("f32_split_64_relu", F32, 450, 130, 72, "split64/0", split=True, bias=True, act=RELU),
    case("f32_split_tiled", F32, 450, 130, 72, "tiled/TR4", split=True, bias=True, act=GELU),
    case("f32x3", F32X3, 300, 128, 64, "split3", stats="rows"),
    case("f32x3_nostats", F32X3, 300, 256, 96, "split3"),
]
# all four a_trans / w_trans combinations on each of the three fp32 kernels, a_rowsum beside a_trans
for _tr in range(1, 4):
    _o = dict(a_trans=bool(_tr & 1), w_trans=bool(_tr & 2))
    CASES += [
        case(f"f32_small_tr{_tr}", F32, 36, 52, 64, f"small/{_tr}", **_o),
        case(f"f32_split64_tr{_tr}", F32, 452, 444, 256, f"split64/{_tr}", split=True, **_o),
        case(f"f32_tiled_tr{_tr}", F32, 1160, 1152, 256, f"tiled/TR{_tr}", **_o),
        case(f"f32_tiled_tr{_tr + 4}", F32, 452, 132, 72, f"tiled/TR{_tr + 4}", split=True, act=GELU, bias=True, **_o),
    ]
CASES += [
    case("f32_rowsum_tiled", F32, 300, 128, 96, "tiled/TR1", a_trans=True, a_rowsum=True),
    case("f32_rowsum_split64", F32, 300, 128, 96, "split64/1", a_trans=True, a_rowsum=True, split=True),
    case("f32_rowsum_tr3", F32, 300, 128, 96, "split64/3", a_trans=True, w_trans=True, a_rowsum=True, split=True),
]

# ---- padded, mutually different leading dimensions, one case per route: lda = K + p, ldw = K + 2p, ldc = N + p, ldr = N + 3p,
#      ldg = N + 2p, lda2 = K2 + p, ldw2 = K2 + 2p; pad="g": p = one 16-byte granule (the route of the dense twin is kept),
#      an odd p takes the tiled kernel's element-wise path (vec_in / vec_out false)
CASES += [
    case("g8_conv_ld", BF16, 12288, 512, 512, "8w/0", stats="rows", pad="g"),
    case("g8_lin_res_ld", BF16, 12288, 512, 512, "8w/1", bias=True, residual=True, pad="g"),
    case("pro_bn_ld", BF16, 32768, 256, 128, "pro", stats="rows", prologue="bn_relu", pad="g"),
    case("pro_tail_ld", BF16, 4096, 256, 128, "pro", prologue="bn_relu", tail=True, residual=True, act=RELU, pad="g"),
    case("glds0_ld", BF16, 1000, 256, 64, "glds/0", stats="rows", pad="g"),
    case("glds1_ld", BF16, 300, 128, 64, "glds/1", bias=True, residual=True, pad="g"),
    case("glds2_ld", BF16, 1000, 256, 64, "glds/2", tail=True, residual=True, act=RELU, pad="g"),
    case("glds6_ld", BF16, 300, 128, 64, "glds/6", G=True, pad="g"),
    case("tiled_bf16_ld", BF16, 300, 120, 96, "tiled/0", bias=True, residual=True, pad="g"),
    case("tiled_f32_ld", F32, 300, 128, 96, "tiled/0", residual=True, pad="g"),
    case("f32_small_ld", F32, 33, 50, 64, "small/0", bias=True, exp_scale=True, pad="g"),
    case("f32_split64_ld", F32, 450, 130, 72, "split64/0", split=True, bias=True, act=RELU, pad="g"),
    case("f32_tiled_tr3_ld", F32, 1160, 1152, 256, "tiled/TR3", a_trans=True, w_trans=True, pad="g"),
    case("tiled_bf16_oddld", BF16, 300, 120, 96, "tiled/0", bias=True, residual=True, pad=3),
    case("tiled_f32_oddld", F32, 300, 128, 96, "tiled/0", residual=True, pad=3),
    # ---- 8-wave ragged last tiles at the threshold: 48 tiles of 256 rows, 56 of 224 (the linear epilogue's cost rule picks 224)
    case("g8_conv_ragged", BF16, 12283, 512, 512, "8w/0", stats="rows"),
    case("g8_lin_ragged224", BF16, 12541, 512, 512, "8w/1", bias=True, residual=True, tile_rows=224),
    # ---- QuickGELU through the dispatcher
    case("glds7_quick", BF16, 300, 128, 64, "glds/7", bias=True, act=QUICK),
    case("g8_lin_quick", BF16, 12288, 512, 512, "8w/1", bias=True, act=QUICK),
    case("tiled_bf16_quick", BF16, 300, 120, 96, "tiled/0", bias=True, act=QUICK),
    case("tiled_f32_quick", F32, 300, 120, 96, "tiled/0", bias=True, act=QUICK),
    # ---- streaming kernel: fewer rows than one 64-row tile; the tail with the downsample branch recomputed
    case("pro_bn_63rows", BF16, 63, 256, 128, "pro", stats="rows", prologue="bn_relu"),
    case("pro_tail_ds", BF16, 4101, 256, 128, "pro", prologue="bn_relu", tail=True, ds=True, act=RELU),
    case("pro_tail_ds_ld", BF16, 4101, 256, 128, "pro", prologue="bn_relu", tail=True, ds=True, act=RELU, pad="g"),
    # ---- instantiations a kernel trace of the cases above did not reach.  8-wave 256-row tiles: every M = 12288 block takes 224-row
    #      tiles on 256 CUs; 29 x 8 tiles of 256 rows fill one round where 33 x 8 of 224 need two (ragged: 7169 = 28 * 256 + 1).
    #      LayerNorm consumer without GELU (the only forms the integer family can run); streaming kernel at K = 256, statistics only / tail
    case("g8_conv_tall", BF16, 7169, 2048, 256, "8w/0", stats="rows", tile_rows=256),
    case("g8_tall_ln_relu", BF16, 7169, 2048, 256, "8w/1", bias=True, act=RELU, ln="consumer"),
    case("g8_tall_row_part", BF16, 7169, 2048, 256, "8w/1", bias=True, residual=True, ln="producer"),
    case("g8_ln_none", BF16, 12288, 512, 512, "8w/1", bias=True, ln="consumer"),
    case("g8_ln_relu", BF16, 12288, 512, 512, "8w/1", bias=True, act=RELU, ln="consumer"),
    case("pro_bn_statsonly_k256", BF16, 4101, 256, 256, "pro", stats="rows", prologue="bn_relu", no_C=True),
    case("pro_tail_k256", BF16, 4101, 256, 256, "pro", prologue="bn_relu", tail=True, residual=True, act=RELU),
    # ---- centred storage on every kernel that honours it (g8_conv_centre above has the 8-wave one); ragged M behind a BN operand
    case("glds0_centre", BF16, 1000, 256, 64, "glds/0", stats="rows", centre=True),
    case("glds2_tail_centre", BF16, 1000, 256, 64, "glds/2", tail=True, residual=True, act=RELU, centre=True),
    case("pro_bn_centre", BF16, 32801, 256, 128, "pro", stats="rows", prologue="bn_relu", centre=True),
    case("pro_tail_centre", BF16, 4101, 256, 128, "pro", prologue="bn_relu", tail=True, residual=True, act=RELU, centre=True),
    case("tiled_bf16_centre", BF16, 300, 128, 96, "tiled/0/lean", stats="rows", centre=True),
    case("tiled_bf16_p2_centre", BF16, 300, 128, 64, "tiled/2/lean", prologue="bn_relu", stats="rows", centre=True),
    case("tiled_f32_centre", F32, 300, 128, 96, "tiled/0/lean", stats="rows", centre=True),
    # ---- tiny, exp_scale on the bf16 tiled kernel, gathers
    case("tiled_bf16_tiny", BF16, 1, 5, 8, "tiled/0", bias=True, act=RELU),
    case("tiled_f32_tiny", F32, 1, 5, 8, "tiled/0", bias=True, act=RELU),
    case("tiled_bf16_expscale", BF16, 33, 50, 64, "tiled/0", bias=True, exp_scale=True),
    case("glds0_gather", BF16, 2 * 49, 128, 64, "glds/0", stats="rows", gather=(7, 7, 14, 14, 2)),
    case("tiled_f32_gather_odd", F32, 2 * 64, 128, 96, "tiled/0/lean", stats="rows", gather=(8, 8, 15, 15, 2)),
]

# ---- every refusal of cvcl_gemm (text as left in cvcl_last_error); none of them needs a device: plan_gemm decides them before any
#      pointer is used or anything is launched (without a device its occupancy / CU-count queries fall back to fixed values)
REFUSALS = [
    case("r_null", BF16, 64, 128, 64, None, null_A=True, refuse="cvcl_gemm: null operand"),
    case("r_dtype", 9, 64, 128, 64, None, refuse="cvcl_gemm: unknown dtype 9"),
    case("r_ln_shape", BF16, 300, 512, 512, None, bias=True, ln="consumer", refuse=LN_MSG.format(M=300, N=512, K=512)),
    case("r_ln_f32", F32, 12288, 512, 512, None, bias=True, ln="consumer", refuse=LN_MSG.format(M=12288, N=512, K=512)),
    case("r_rowpart_nores", BF16, 12288, 512, 512, None, bias=True, ln="producer", refuse=LN_MSG.format(M=12288, N=512, K=512)),
    case("r_colsum_only", BF16, 300, 512, 512, None, bias=True, ln="colsum", refuse=LN_MSG.format(M=300, N=512, K=512)),
    case("r_c_scale_f32", F32, 300, 256, 64, None, tail=True, residual=True, act=RELU, refuse="cvcl_gemm: the c_scale epilogue exists for bf16 only"),
    case("r_shape", BF16, 0, 128, 64, None, refuse="cvcl_gemm: bad shape 0 128 64"),
    case("r_shape_n0", BF16, 64, 0, 64, None, refuse="cvcl_gemm: bad shape 64 0 64"),
    case("r_shape_k0", F32, 64, 128, 0, None, refuse="cvcl_gemm: bad shape 64 128 0"),
    case("r_shape_n0_big", BF16, 12288, 0, 512, None, bias=True, refuse="cvcl_gemm: bad shape 12288 0 512"),
    case("r_shape_neg", F32, 300, -128, 64, None, refuse="cvcl_gemm: bad shape 300 -128 64"),
    case("r_ln_n0", BF16, 12288, 0, 512, None, bias=True, ln="consumer", refuse=LN_MSG.format(M=12288, N=0, K=512)),
    case("r_scale_alone", BF16, 300, 128, 64, None, prologue="scale_only", refuse="cvcl_gemm: a_scale/a_shift must come together"),
    case("r_centre_bias", BF16, 300, 128, 64, None, centre=True, bias=True,
         refuse="cvcl_gemm: centre goes with the convolution epilogues only (16-byte aligned, no bias / activation / residual)"),
    case("r_tr_bf16", BF16, 300, 128, 64, None, a_trans=True, refuse="cvcl_gemm: a_trans / w_trans / a_rowsum / f32_split are fp32 options"),
    case("r_rowsum_alone", F32, 300, 128, 64, None, a_rowsum=True,
         refuse="cvcl_gemm: a_rowsum goes with a_trans (the bias gradient beside dW = dY^T X)"),
    case("r_tr_stats", F32, 300, 128, 64, None, w_trans=True, stats="rows",
         refuse="cvcl_gemm: K-major operands / split arithmetic take no prologue / gather / statistics / BN-tail options"),
    case("r_tail_bias", BF16, 300, 256, 64, None, tail=True, residual=True, bias=True, act=RELU,
         refuse="cvcl_gemm: the c_scale epilogue needs bf16, K % 64 == 0, N % 128 == 0, a residual and no bias/stats"),
    case("r_c_pre_k", BF16, 300, 128, 96, None, bias=True, act=GELU, C_pre=True,
         refuse="cvcl_gemm: the C_pre / G epilogues need bf16, K % 64 == 0, N % 128 == 0 and 16-byte aligned rows"),
    case("r_c_pre_act", BF16, 300, 128, 64, None, bias=True, act=RELU, C_pre=True, refuse="cvcl_gemm: C_pre goes with act = GELU and no residual"),
    case("r_g_bias", BF16, 300, 128, 64, None, bias=True, G=True, refuse="cvcl_gemm: G (GELU-backward epilogue) takes no bias / activation / residual"),
    case("r_statsonly_f32", F32, 300, 128, 64, None, stats="rows", no_C=True,
         refuse="cvcl_gemm: statistics-only / BN-tail epilogues need the direct-to-LDS bf16 path"),
]


def itemsize(dt):
    return 2 if dt == BF16 else 4


def pad_of(c):
    """p of a case's padded leading dimensions in elements (0: dense); "g" is one 16-byte granule of the storage type"""
    p = c.get("pad", 0)
    return 16 // itemsize(c["dt"]) if p == "g" else p


def stats_rows(lib, c):
    """rows of the statistics buffer the case passes (cvcl_gemm_stats_rows on the block without one; "short": one fewer)"""
    n = lib.cvcl_gemm_stats_rows(c["dt"], C.byref(build_args(lib, dict(c, stats=None), lambda *a: DUMMY)))
    return n - 1 if c.get("stats") == "short" else n


def build_args(lib, c, alloc):
    """cvcl_gemm_args of a case.  alloc(name, shape, kind, ld) -> pointer; kind "op" / "w" (the case's storage dtype), "f32" or "i64";
    shape is the logical shape and ld the leading dimension in elements of a 2-D operand (None: dense)."""
    M, N, K, dt, p = c["M"], c["N"], c["K"], c["dt"], pad_of(c)
    a = H.GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.a_trans, a.w_trans, a.f32_split = int(c.get("a_trans", False)), int(c.get("w_trans", False)), int(c.get("split", False))
    g = c.get("gather")
    a_rows = M if not g else M // (g[0] * g[1]) * g[2] * g[3]
    a.lda, a.ldw, a.ldc = (M if a.a_trans else K) + p, (N if a.w_trans else K) + 2 * p, N + p
    a.A = None if c.get("null_A") else alloc("A", (K, M) if a.a_trans else (a_rows, K), "op", a.lda)
    a.W = alloc("W", (K, N) if a.w_trans else (N, K), "w", a.ldw)
    if not c.get("no_C"):
        a.C = alloc("C", (M, N), "op", a.ldc)
    if g:
        a.gather_ho, a.gather_wo, a.gather_hi, a.gather_wi, a.gather_stride = g
    pro = c.get("prologue")
    if pro:
        a.a_scale = alloc("a_scale", (K,), "f32", None)
        if pro != "scale_only":
            a.a_shift = alloc("a_shift", (K,), "f32", None)
        a.a_relu = int(pro == "bn_relu")
    if c.get("bias"):
        a.bias = alloc("bias", (N,), "f32", None)
    if c.get("exp_scale"):
        a.exp_scale = alloc("exp_scale", (1,), "f32", None)
    a.act = c.get("act", NONE)
    if c.get("residual"):
        a.ldr = N + 3 * p
        a.R = alloc("R", (M, N), "op", a.ldr)
    if c.get("tail"):
        a.c_scale, a.c_shift = alloc("c_scale", (N,), "f32", None), alloc("c_shift", (N,), "f32", None)
        if c.get("r_scale") or c.get("ds"):
            a.r_scale, a.r_shift = alloc("r_scale", (N,), "f32", None), alloc("r_shift", (N,), "f32", None)
    if c.get("ds"):                                            # the downsample branch recomputed from the block input (K2 = 64)
        a.K2, a.lda2, a.ldw2 = 64, 64 + p, 64 + 2 * p
        a.A2, a.W2 = alloc("A2", (M, 64), "op", a.lda2), alloc("W2", (N, 64), "w", a.ldw2)
        a.centre2 = alloc("centre2", (N,), "f32", None)
    if c.get("C_pre"):
        a.C_pre = alloc("C_pre", (M, N), "op", a.ldc)
    if c.get("G"):
        a.ldg = N + 2 * p
        a.G = alloc("G", (M, N), "op", a.ldg)
    if c.get("centre"):
        a.centre = alloc("centre", (N,), "f32", None)
    ln = c.get("ln")
    if ln in ("consumer", "colsum"):
        a.ln_colsum = alloc("ln_colsum", (N,), "f32", None)
        if ln == "consumer":
            a.ln_stats = alloc("ln_stats", (M + (M & 1), 2), "f32", None)
    if ln == "producer":
        a.row_part = alloc("row_part", (M, N // 64, 2), "f32", None)
    if c.get("a_rowsum"):
        a.a_rowsum = alloc("a_rowsum", (M,), "f32", None)
    st = c.get("stats")
    if st == "acc":
        a.stats, a.stats_rows = alloc("stats", (8, 2, N), "i64", None), H.STATS_ACCUMULATE
    elif st:
        rows = stats_rows(lib, c)
        a.stats, a.stats_rows = alloc("stats", (rows + 1, 2, N), "f32", None), rows      # (one spare row: what a kernel must not touch)
    return a


OUTPUTS = ("C", "C_pre", "stats", "row_part", "a_rowsum")
FAMILIES = ("random", "integer")
PAD_FILL = 32768.0       # what the padding columns of an INPUT hold: finite, exact in bf16, and far outside every value of a case
CANARY = -0x5A5A5A5A5A5A5A5B                                  # the guard row behind the int64 accumulators
GUARD = 64               # guard elements behind a_rowsum / row_part / C / C_pre (beside one extra row and the padding columns)


def in_integer_family(c):
    """the integer family has no exact form of GELU / QuickGELU, C_pre or G"""
    return c.get("act", NONE) in (NONE, RELU) and not c.get("C_pre") and not c.get("G")


def make_inputs(lib, c, family="random", seed=0):
    """The input tensors of a case on the CPU, in their logical (dense) shapes, seeded per case tag.

    random:  normal operands; scales |x| + 0.5; ln_stats[m] = (rstd > 0, -mean rstd); exp_scale ~ 0.1.
    integer: everything a correct kernel computes is an integer that bf16 and any fp32 partial sum hold exactly: A, W (A2, W2)
             sparse in {-1, 0, 1} with density 2 / sqrt(K) (about four non-zero products per output element), R in [-3, 3], bias /
             shifts / centres / ln_colsum in [-2, 2], every scale 1 or 2, exp_scale 0, ln_stats = (1 | 2, -1 | 0 | 1).
    (CVCL_F32X3: W is the fp32 source here; GpuBlock packs it.)"""
    import zlib

    import torch
    assert family in FAMILIES
    shapes = []
    build_args(lib, c, lambda name, shape, kind, ld: shapes.append((name, shape, kind)) or DUMMY)
    gen = torch.Generator().manual_seed(zlib.crc32(c["tag"].encode()) + seed)
    op = torch.bfloat16 if c["dt"] == BF16 else torch.float32
    t = {}
    for name, shape, kind in shapes:
        if name in OUTPUTS:
            continue
        if family == "random":
            x = torch.randn(shape, generator=gen, dtype=torch.float32)
            if name == "ln_stats":
                x[:, 0] = x[:, 0].abs() + 0.5
            if name in ("a_scale", "c_scale", "r_scale"):
                x = x.abs() + 0.5
            if name == "exp_scale":
                x = x * 0.1
        else:
            def ints(lo, hi, shape=shape):
                return torch.randint(lo, hi + 1, shape, generator=gen).float()
            if name in ("A", "W", "A2", "W2"):
                k = c["K"] if name in ("A", "W") else 64
                keep = torch.rand(shape, generator=gen) < min(1.0, 2.0 / k ** 0.5)
                x = (ints(0, 1) * 2 - 1) * keep
            elif name in ("a_scale", "c_scale", "r_scale"):
                x = 2.0 ** ints(0, 1)
            elif name == "a_shift":
                x = ints(-1, 1) * (torch.rand(shape, generator=gen) < 0.25)
            elif name == "exp_scale":
                x = torch.zeros(shape)
            elif name == "ln_stats":
                x = torch.stack([2.0 ** ints(0, 1, shape[:1]), ints(-1, 1, shape[:1])], dim=1)
            elif name in ("R", "G"):
                x = ints(-3, 3)
            else:                                              # bias, c_shift, r_shift, centre, centre2, ln_colsum
                x = ints(-2, 2)
        t[name] = x.to(op) if kind in ("op", "w") and not (kind == "w" and c["dt"] == F32X3) else x
    return t


def pack_f32x3_host(w):
    """what cvcl_pack_conv_weight(CVCL_F32X3, CVCL_PACK_DENSE) writes for w [N][K], for blocks built without a device:
    three bf16 parts [3][N][K], x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1) (the layout csrc/gemm_split.hip documents)"""
    import torch
    parts, r = [], w.clone()
    for _ in range(3):
        parts.append(r.to(torch.bfloat16))
        r = r - parts[-1].float()
    return torch.stack(parts).contiguous().view(torch.uint8).reshape(-1)


class GpuBlock:
    """Device tensors of a case: ``args`` is the block, ``t`` maps operand names to the buffers the block points to (outputs start
    as NaN, the int64 accumulators as zero), ``inputs`` the logical input tensors on the CPU (make_inputs).

    guard: every output buffer gets one extra row, its padding columns [N, ldc) and GUARD elements behind it, all NaN (the
    accumulators one more row of CANARY); ``split_output`` separates what a call may write from what it must not.
    device="cpu" builds the same block in host memory (for a float32 evaluation of the contract, not for the library)."""
    OUTPUTS = OUTPUTS

    def __init__(self, lib, c, seed=0, family="random", guard=False, device="cuda", inputs=None):
        import torch
        self.c, self.t, self.meta, dt = c, {}, {}, c["dt"]
        self.inputs = inputs if inputs is not None else make_inputs(lib, c, family, seed)
        op = torch.bfloat16 if dt == BF16 else torch.float32

        def alloc(name, shape, kind, ld):
            self.meta[name] = (shape, ld if ld is not None and len(shape) == 2 else None, kind)
            if kind == "i64":
                t = torch.zeros((shape[0] + int(guard),) + shape[1:], dtype=torch.int64, device=device)
                if guard:
                    t[-1] = CANARY
            elif name in OUTPUTS:
                ty = op if kind == "op" else torch.float32
                if name == "stats":                            # (build_args has given it its spare row)
                    t = torch.full(shape, float("nan"), dtype=ty, device=device)
                else:
                    n = shape[0] * ld if self.meta[name][1] else int(torch.Size(shape).numel())
                    n += ((ld if self.meta[name][1] else 0) + GUARD) if guard else 0
                    t = torch.full((n,), float("nan"), dtype=ty, device=device)
                    if not guard:
                        t = t.view(shape[0], ld) if self.meta[name][1] else t.view(shape)
            else:
                t = self.inputs[name]
                if kind == "w" and dt == F32X3:                # the 3-term library reads W as packed bf16 parts
                    n, k = shape
                    if device == "cpu":
                        t = pack_f32x3_host(t)
                    else:
                        src = t.to(device)
                        t = torch.empty(lib.cvcl_packed_weight_bytes(F32X3, H.PACK_DENSE, n, k, 1), dtype=torch.uint8, device=device)
                        H.check(lib.cvcl_pack_conv_weight(F32X3, H.PACK_DENSE, src.data_ptr(), t.data_ptr(), n, k, 1, H.stream_ptr()), "pack")
                        torch.cuda.synchronize()
                elif self.meta[name][1] and ld > shape[1]:
                    buf = torch.full((shape[0], ld), PAD_FILL, dtype=t.dtype)
                    buf[:, :shape[1]] = t
                    t = buf.to(device)
                else:
                    t = t.to(device).contiguous()
            self.t[name] = t
            return t.data_ptr()

        self.guard = guard
        self.args = build_args(lib, c, alloc)

    def outputs(self):
        return {k: v for k, v in self.t.items() if k in OUTPUTS}

    def ref_inputs(self):
        """the inputs as the reference takes them: logical CPU tensors; CVCL_F32X3: W as the packed bytes the block points to"""
        t = dict(self.inputs)
        if self.c["dt"] == F32X3:
            t["W"] = self.t["W"].cpu()
        return t

    def split_output(self, name):
        """(values, guard) of an output of a guarded block, both on the CPU: the logical tensor a call may write, and a flat
        tensor of everything else in the buffer (extra row, padding columns, guard elements), which it must leave alone"""
        import torch
        assert self.guard
        shape, ld, kind = self.meta[name]
        buf = self.t[name].cpu()
        if name == "stats":                                    # f32 rows + the spare row | accumulators + the canary row
            return buf.view((-1,) + shape[1:])[:-1], buf.view((-1,) + shape[1:])[-1].reshape(-1)
        if ld:
            body = buf[:(shape[0] + 1) * ld].view(shape[0] + 1, ld)
            return body[:shape[0], :shape[1]], torch.cat([body[:shape[0], shape[1]:].reshape(-1), body[shape[0]].reshape(-1), buf[(shape[0] + 1) * ld:]])
        n = int(torch.Size(shape).numel())
        return buf[:n].view(shape), buf[n:]
