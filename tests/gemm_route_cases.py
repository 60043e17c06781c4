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
NONE, RELU, GELU = H.ACT_NONE, H.ACT_RELU, H.ACT_GELU
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


def stats_rows(lib, c):
    """rows of the statistics buffer the case passes (cvcl_gemm_stats_rows on the block without one; "short": one fewer)"""
    n = lib.cvcl_gemm_stats_rows(c["dt"], C.byref(build_args(lib, dict(c, stats=None), lambda *a: DUMMY)))
    return n - 1 if c.get("stats") == "short" else n


def build_args(lib, c, alloc):
    """cvcl_gemm_args of a case.  alloc(name, shape, kind) -> pointer, kind "op" (the case's storage dtype), "f32" or "i64"."""
    M, N, K, dt = c["M"], c["N"], c["K"], c["dt"]
    a = H.GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.a_trans, a.w_trans, a.f32_split = int(c.get("a_trans", False)), int(c.get("w_trans", False)), int(c.get("split", False))
    g = c.get("gather")
    a_rows = M if not g else M // (g[0] * g[1]) * g[2] * g[3]
    a.A = None if c.get("null_A") else alloc("A", (K, M) if a.a_trans else (a_rows, K), "op")
    a.W = alloc("W", (K, N) if a.w_trans else (N, K), "w")
    a.lda, a.ldw, a.ldc = (M if a.a_trans else K), (N if a.w_trans else K), N
    if not c.get("no_C"):
        a.C = alloc("C", (M, N), "op")
    if g:
        a.gather_ho, a.gather_wo, a.gather_hi, a.gather_wi, a.gather_stride = g
    pro = c.get("prologue")
    if pro:
        a.a_scale = alloc("a_scale", (K,), "f32")
        if pro != "scale_only":
            a.a_shift = alloc("a_shift", (K,), "f32")
        a.a_relu = int(pro == "bn_relu")
    if c.get("bias"):
        a.bias = alloc("bias", (N,), "f32")
    if c.get("exp_scale"):
        a.exp_scale = alloc("exp_scale", (1,), "f32")
    a.act = c.get("act", NONE)
    if c.get("residual"):
        a.R, a.ldr = alloc("R", (M, N), "op"), N
    if c.get("tail"):
        a.c_scale, a.c_shift = alloc("c_scale", (N,), "f32"), alloc("c_shift", (N,), "f32")
        if c.get("r_scale"):
            a.r_scale, a.r_shift = alloc("r_scale", (N,), "f32"), alloc("r_shift", (N,), "f32")
    if c.get("C_pre"):
        a.C_pre = alloc("C_pre", (M, N), "op")
    if c.get("G"):
        a.G, a.ldg = alloc("G", (M, N), "op"), N
    if c.get("centre"):
        a.centre = alloc("centre", (N,), "f32")
    ln = c.get("ln")
    if ln in ("consumer", "colsum"):
        a.ln_colsum = alloc("ln_colsum", (N,), "f32")
        if ln == "consumer":
            a.ln_stats = alloc("ln_stats", (M + (M & 1), 2), "f32")
    if ln == "producer":
        a.row_part = alloc("row_part", (M, N // 64, 2), "f32")
    if c.get("a_rowsum"):
        a.a_rowsum = alloc("a_rowsum", (M,), "f32")
    st = c.get("stats")
    if st == "acc":
        a.stats, a.stats_rows = alloc("stats", (8, 2, N), "i64"), H.STATS_ACCUMULATE
    elif st:
        rows = stats_rows(lib, c)
        a.stats, a.stats_rows = alloc("stats", (rows + 1, 2, N), "f32"), rows      # (one spare row: what a kernel must not touch)
    return a


class GpuBlock:
    """Seeded device tensors of a case: ``args`` is the block, ``t`` maps operand names to tensors (outputs start as NaN / zero)."""
    OUTPUTS = ("C", "C_pre", "stats", "row_part", "a_rowsum")

    def __init__(self, lib, c, seed=0):
        import torch
        self.t, dt = {}, c["dt"]
        gen = torch.Generator(device="cuda").manual_seed(seed)
        op = torch.bfloat16 if dt == BF16 else torch.float32

        def alloc(name, shape, kind):
            if kind == "i64":
                t = torch.zeros(shape, dtype=torch.int64, device="cuda")
            elif name in self.OUTPUTS:
                t = torch.full(shape, float("nan"), dtype=op if kind == "op" else torch.float32, device="cuda")
            else:
                t = torch.randn(shape, generator=gen, device="cuda", dtype=torch.float32)
                if name == "ln_stats":                         # (mean, rstd) per row
                    t[:, 1] = t[:, 1].abs() + 0.5
                if name in ("a_scale", "c_scale", "r_scale"):
                    t = t.abs() + 0.5
                if name == "exp_scale":
                    t = t * 0.1
                if kind == "w" and dt == F32X3:                # the 3-term library reads W as packed bf16 parts
                    n, k = shape
                    packed = torch.empty(lib.cvcl_packed_weight_bytes(F32X3, H.PACK_DENSE, n, k, 1), dtype=torch.uint8, device="cuda")
                    H.check(lib.cvcl_pack_conv_weight(F32X3, H.PACK_DENSE, t.data_ptr(), packed.data_ptr(), n, k, 1, H.stream_ptr()), "pack")
                    t = packed
                elif kind in ("op", "w"):
                    t = t.to(op)
            self.t[name] = t
            return t.data_ptr()

        self.args = build_args(lib, c, alloc)

    def outputs(self):
        return {k: v for k, v in self.t.items() if k in self.OUTPUTS}
