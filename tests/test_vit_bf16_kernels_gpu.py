"""GPU: the bf16 ViT fine-tuning kernels, one by one, against float64 on the CPU computed from the bf16-rounded inputs the kernel
receives -- the LayerNorm backward on bf16 rows (every template instantiation, the second trip of its row loop, strided rows), the
fused weight / bias gradient (exact on small integers), the token backward (batch tails, grid-stride trips), GELU forward / backward
over every finite bf16 value, and the attention forward / backward at the limits of T.  Every output and workspace starts as NaN
(or a canary), every kernel runs twice and must repeat itself bit for bit, and a refused call leaves its outputs untouched."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
EINVAL, EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    _hip.load()
    return _hip


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---- 1. LayerNorm backward ---------------------------------------------------------------------------------------------------------

def ln_bwd_ref(x, dy, gamma, add, eps):
    """float64 LayerNorm backward of rows x [rows, D]: -> (dx (+ add), s, dgamma, dbeta); s is the sum of the magnitudes of the
    terms of dx, the scale of the fp32 rounding floor of the bound."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    xc = x - x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xh = xc * rstd
    g = dy * gamma
    mg, mgx = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    a = add.double() if add is not None else torch.zeros_like(x)
    dx = rstd * (g - mg - xh * mgx) + a
    s = rstd * (g.abs() + mg.abs() + (xh * mgx).abs()) + a.abs()
    return dx, s, (dy * xh).sum(0), dy.sum(0)


def ln_case(H, dev, rows, D, dy_f32, with_add, strided):
    torch.manual_seed(rows * 7 + D + int(dy_f32))
    xs = 3 * D if strided else D                      # strided rows: the final norm reads the cls rows of [B][T][D]
    x = (torch.randn(rows, xs) * 2 + 0.5).to(BF)
    dy = torch.randn(rows, D) + 0.5                   # non-zero mean: mean(g) carries weight in dx
    if not dy_f32:
        dy = dy.to(BF)
    gamma = torch.rand(D) + 0.5
    add = torch.randn(rows, xs).to(BF) if with_add else None
    dx_ref, s, dg_ref, db_ref = ln_bwd_ref(x[:, :D], dy, gamma, add[:, :D] if with_add else None, 1e-6)
    lib, st = H.lib(), H.stream_ptr()
    npart = lib.cvcl_layernorm_bwd_rows_partials(rows)
    assert npart == 8 * min(768, (rows + 7) // 8)
    xd, dyd, gd, addd = x.to(dev), dy.to(dev), gamma.to(dev), add.to(dev) if with_add else None
    fill = 5.0 if strided else NAN
    runs = []
    for _ in range(2):
        dx = torch.full((rows, xs), fill, dtype=BF, device=dev)
        part = torch.full((npart, 2 * D), NAN, device=dev)
        red = torch.full((2 * D,), NAN, device=dev)
        H.check(lib.cvcl_layernorm_bwd_rows(H.ptr(xd), xs, H.ptr(gd), H.ptr(dyd), int(dy_f32), D, 1e-6, H.ptr(addd), H.ptr(dx), xs,
                                            H.ptr(part), rows, D, st), "cvcl_layernorm_bwd_rows")
        H.check(lib.cvcl_colsum_f32(H.ptr(part), H.ptr(red), npart, 2 * D, st), "cvcl_colsum_f32")
        torch.cuda.synchronize()
        runs.append((dx.cpu(), part.cpu(), red.cpu()))
    dx, part, red = runs[0]
    assert torch.isfinite(dx.float()).all() and torch.isfinite(part).all() and torch.isfinite(red).all()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    if rows < npart:                                  # row groups without a row write zero partials
        assert bool((part[rows:] == 0).all())
    err = (dx[:, :D].double() - dx_ref).abs()
    bound = 2.0 ** -7 * dx_ref.abs() + 2.0 ** -18 * s
    e_g, e_b = rel_l2(red[:D], dg_ref), rel_l2(red[D:], db_ref)
    print(f"LN bwd bf16 rows {rows} D {D} dy {'f32' if dy_f32 else 'bf16'} add {with_add} strided {strided}: "
          f"dx max err/bound {float((err / bound).max()):.3f}  dgamma rel-L2 {e_g:.2e}  dbeta rel-L2 {e_b:.2e}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements of dx outside the bound"
    assert e_g < 2e-6 and e_b < 2e-6
    if strided:                                       # the columns between the rows are not written
        assert bool((dx[:, D:] == 5.0).all())


LN_CASES = [(1001, 768, False, True), (517, 128, False, True), (300, 1024, False, True), (64, 776, False, True),
            (6157, 768, False, True), (6157, 8, False, True), (1, 384, False, True),
            (1001, 768, True, True), (300, 1024, True, True), (517, 128, True, True),
            (517, 128, False, False)]


@pytest.mark.parametrize("rows,D,dy_f32,with_add", LN_CASES)
def test_layernorm_bwd_rows_bf16_vs_float64(H, dev, rows, D, dy_f32, with_add):
    """cvcl_layernorm_bwd_rows + cvcl_colsum_f32 over its partials.  The four instantiations: bf16 dy at D == 768 (EXACT), D < 768,
    768 < D <= 1024 (1024 and the ragged 776), fp32 dy at any D; 6157 rows > 768 workgroups x 8 groups = the second trip of the
    row loop; D = 8 leaves 31 of a row's 32 lanes idle; 1 row leaves 7 row groups idle (zero partials).
    dx, every element: |got - ref| <= 2^-7 |ref| + 2^-18 s, s = rstd (|g| + |mean g| + |xhat mean(g xhat)|) + |add| -- 2^-8 is the
    worst-case rounding to bf16, the second 2^-8 and the fp32 floor leave room for a different fp32 summation order that flips a
    rounding; dropping mean(g) or mean(g xhat) misses it by factors of 1e3 to 1e5.
    dgamma / dbeta: rel-L2 < 2e-6, the bound of the fp32 sibling (the arithmetic after the load is the same fp32); measured on
    the MI355X: at most 4.3e-7 (dgamma, 6157 x 768) and 1.3e-7 (dbeta) over these cases; dx reaches 0.498 of its bound at most."""
    ln_case(H, dev, rows, D, dy_f32, with_add, strided=False)


def test_layernorm_bwd_rows_bf16_strided_final_norm(H, dev):
    """The final norm's call: 5 cls rows at stride 3 D inside [B][T][D], fp32 dy at stride D, no residual add; the columns of dx
    between the rows keep their canary.  Bounds as test_layernorm_bwd_rows_bf16_vs_float64."""
    ln_case(H, dev, 5, 384, True, False, strided=True)


def test_layernorm_bwd_rows_bf16_refusals_leave_outputs_untouched(H, dev):
    lib, st = H.lib(), H.stream_ptr()
    rows, W = 10, 1040
    x = torch.zeros(rows * W, dtype=BF, device=dev)
    dy = torch.zeros(rows * W, device=dev)               # read as bf16 or fp32: large enough for both
    gamma = torch.ones(W, device=dev)
    dx = torch.full((rows * W,), 7.0, dtype=BF, device=dev)
    part = torch.full((lib.cvcl_layernorm_bwd_rows_partials(rows) * 2 * W,), 7.0, device=dev)
    p = H.ptr

    def call(xs, dy_f32, dys, dxs, D, partial=part):
        return lib.cvcl_layernorm_bwd_rows(p(x), xs, p(gamma), p(dy), dy_f32, dys, 1e-6, None, p(dx), dxs, p(partial), rows, D, st)
    assert call(1032, 0, 1032, 1032, 1032) != 0          # D > 1024
    assert call(16, 0, 16, 16, 12) != 0                  # D % 8
    assert call(768 + 4, 0, 768, 768, 768) != 0          # x rows not 16-byte aligned
    assert call(768, 1, 768 + 2, 768, 768) != 0          # fp32 dy rows not 16-byte aligned
    assert call(768, 0, 768, 768, 768, partial=None) != 0
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((part == 7.0).all())


# ---- 2. fused weight / bias gradient -----------------------------------------------------------------------------------------------

def int_operand(M, cols, ld):
    """bf16 [M, ld] holding integers in [-3, 3] in its first `cols` columns and NaN in the padding between the rows."""
    t = torch.full((M, ld), NAN)
    t[:, :cols] = torch.randint(-3, 4, (M, cols)).float()
    return t.to(BF)


# (M, N, K, k_keep, lda - N, ldb - K, splits S of tn_plan)
TN_CASES = [(7, 128, 128, 128, 0, 0, 1),                # less than one 64-row step
            (1000, 200, 328, 321, 0, 0, 1),             # ragged N and K tiles; 3 K tiles share one set of column sums
            (3000, 128, 128, 128, 0, 0, 3),             # S = 3: the workgroup-id mapping of S % 8 != 0
            (9221, 128, 128, 128, 0, 0, 16),            # 15 splits of 640 rows padded to 16: one empty split, the S % 8 == 0 mapping
            (5000, 384, 136, 130, 8, 16, 5)]            # strided views


@pytest.mark.parametrize("M,N,K,k_keep,pad_a,pad_b,S", TN_CASES)
def test_gemm_tn_colsum_bf16_exact_on_integers(H, dev, M, N, K, k_keep, pad_a, pad_b, S):
    """cvcl_gemm_tn_colsum on integers in [-3, 3]: every partial sum is exact in fp32 (|sum| <= 9 * 9221 < 2^24), so dW must equal
    the int64 (A^T B)[:, :k_keep] and db the int64 column sums, exactly; dW must also be bit-equal to cvcl_gemm_tn's (same plan,
    same kernel).  The workspace is sized by the entry's own query and starts as NaN bytes."""
    torch.manual_seed(M + N + K)
    lda, ldb = N + pad_a, K + pad_b
    a, b = int_operand(M, N, lda), int_operand(M, K, ldb)
    ref_w = (a[:, :N].long().t() @ b[:, :K].long())[:, :k_keep]
    ref_b = a[:, :N].long().sum(0)
    lib, st = H.lib(), H.stream_ptr()
    nb = lib.cvcl_gemm_tn_colsum_workspace_bytes(M, N, K)
    assert nb == S * (N * K * 4 + (N + 127) // 128 * 128 * 4)             # S partial matrices + S x tiles_n x 128 column sums
    ad, bd = a.to(dev), b.to(dev)
    runs = []
    for _ in range(2):
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
        dw = torch.full((N, k_keep), NAN, device=dev)
        db = torch.full((N,), NAN, device=dev)
        H.check(lib.cvcl_gemm_tn_colsum(H.ptr(ad), lda, H.ptr(bd), ldb, M, N, K, H.ptr(dw), k_keep, H.ptr(db), H.ptr(ws), nb, st),
                "cvcl_gemm_tn_colsum")
        torch.cuda.synchronize()
        runs.append((dw.cpu(), db.cpu()))
    dw, db = runs[0]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(dw.double(), ref_w.double())
    assert torch.equal(db.double(), ref_b.double())
    nb2 = lib.cvcl_gemm_tn_workspace_bytes(H.BF16, M, N, K)
    ws2 = torch.full((nb2,), 0xFF, dtype=torch.uint8, device=dev)
    dw2 = torch.full((N, k_keep), NAN, device=dev)
    H.check(lib.cvcl_gemm_tn(H.BF16, H.ptr(ad), lda, H.ptr(bd), ldb, M, N, K, H.ptr(dw2), k_keep, H.ptr(ws2), nb2, st), "cvcl_gemm_tn")
    torch.cuda.synchronize()
    assert torch.equal(dw2.cpu(), dw)


def test_gemm_tn_colsum_bf16_refusals_leave_outputs_untouched(H, dev):
    lib, st = H.lib(), H.stream_ptr()
    M = 1000
    a = torch.zeros(M, 136, dtype=BF, device=dev)
    b = torch.zeros(M, 128, dtype=BF, device=dev)
    nb = lib.cvcl_gemm_tn_colsum_workspace_bytes(M, 136, 128)
    ws = torch.full((nb,), 7, dtype=torch.uint8, device=dev)
    dw = torch.full((136, 128), 7.0, device=dev)
    db = torch.full((136,), 7.0, device=dev)
    p = H.ptr
    assert lib.cvcl_gemm_tn_colsum(p(a), 136, p(b), 128, M, 132, 128, p(dw), 128, p(db), p(ws), nb, st) == EINVAL       # N % 8
    assert lib.cvcl_gemm_tn_colsum(p(a), 120, p(b), 128, M, 128, 128, p(dw), 128, p(db), p(ws), nb, st) == EINVAL       # lda < N
    nb128 = lib.cvcl_gemm_tn_colsum_workspace_bytes(M, 128, 128)
    assert lib.cvcl_gemm_tn_colsum(p(a), 136, p(b), 128, M, 128, 128, p(dw), 128, p(db), p(ws), nb128 - 1, st) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((db == 7.0).all()) and bool((ws == 7).all())


# ---- 3. token backward -------------------------------------------------------------------------------------------------------------

# B = 1, 5, 9, 17: the clamped row index of the eight-row batch trips; (2, 8200, 1032): 2 115 342 copy chunks > 8192 x 256 and
# 1 057 800 sum chunks > 4096 x 256 -- both grid-stride loops take a second trip (34 MB of dh)
@pytest.mark.parametrize("B,T,D", [(1, 7, 192), (5, 7, 192), (8, 7, 192), (9, 7, 192), (17, 7, 192), (2, 8200, 1032)])
def test_vit_tokens_bwd_bf16_exact(H, dev, B, T, D):
    """cvcl_vit_tokens_bwd: d_tok is a copy of the patch rows; d_pos is the fp32 sum over the batch in batch order from 0.0f, which
    IEEE arithmetic makes exact against the same running sum on the CPU; it also sits within 1e-6 rel-L2 of the float64 sum."""
    torch.manual_seed(B + T)
    dh = torch.randn(B, T, D).to(BF)
    run = torch.zeros(T, D)
    for b in range(B):
        run += dh[b].float()
    lib, st = H.lib(), H.stream_ptr()
    dhd = dh.to(dev)
    runs = []
    for _ in range(2):
        d_tok = torch.full((B, T - 1, D), NAN, dtype=BF, device=dev)
        d_pos = torch.full((T, D), NAN, device=dev)
        H.check(lib.cvcl_vit_tokens_bwd(H.ptr(dhd), H.ptr(d_tok), H.ptr(d_pos), B, T, D, st), "cvcl_vit_tokens_bwd")
        torch.cuda.synchronize()
        runs.append((d_tok.cpu(), d_pos.cpu()))
    d_tok, d_pos = runs[0]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(d_tok, dh[:, 1:])
    assert torch.equal(d_pos, run)
    assert rel_l2(d_pos, dh.double().sum(0)) < 1e-6


# ---- 4. GELU -----------------------------------------------------------------------------------------------------------------------

GELU_TILES = 258                                       # 258 x 65 280 = 16 842 240 elements > 8192 x 256 x 8: a second grid-stride trip


@pytest.fixture(scope="module")
def gelu_table(H, dev):
    """Every finite bf16 value u (65 280 of them), a random bf16 d_y, the float64 gelu(u), gelu'(u) (Phi through erfc: no
    cancellation in the negative tail) and the kernel's three outputs on that table: gelu(u), 1 * gelu'(u), d_y * gelu'(u)."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    u = (bits - 65536 * (bits >= 32768).int()).to(torch.int16).view(BF)
    assert u.numel() == 65280 and bool(torch.isfinite(u.float()).all())
    torch.manual_seed(11)
    d = torch.randn(u.numel()).to(BF)
    u64 = u.double()
    cdf = 0.5 * torch.special.erfc(-u64 / math.sqrt(2.0))
    ref_y = u64 * cdf
    ref_g = cdf + u64 * torch.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi)
    lib, st = H.lib(), H.stream_ptr()
    ud, dd, one = u.to(dev), d.to(dev), torch.ones(u.numel(), dtype=BF, device=dev)

    def run(d_y):
        outs = []
        for _ in range(2):
            y = torch.full((u.numel(),), NAN, dtype=BF, device=dev)
            H.check(lib.cvcl_gelu_bf16(H.ptr(ud), H.ptr(d_y), H.ptr(y), u.numel(), st), "cvcl_gelu_bf16")
            torch.cuda.synchronize()
            outs.append(y.cpu())
        assert torch.equal(outs[0], outs[1])
        return outs[0]
    return {"u": u, "d": d, "ref_y": ref_y, "ref_g": ref_g, "y": run(None), "g": run(one), "du": run(dd)}


def worst(err, bound, u):
    i = int((err / bound.clamp_min(1e-300)).argmax())
    return f"largest |err| / bound {float(err[i] / bound[i]):.3f} at u = {float(u[i]):.6g} (|err| {float(err[i]):.3e}, bound {float(bound[i]):.3e})"


def beyond_rounding(got, err):
    """The part of |err| that half a bf16 ulp of the value the kernel returned cannot explain: a lower bound of the error of the
    fp32 value before it was rounded."""
    half_ulp = torch.ldexp(torch.ones_like(got), torch.frexp(got)[1] - 9)          # got = m 2^e, 0.5 <= |m| < 1: ulp = 2^(e - 8)
    return (err - torch.where(got == 0, torch.zeros_like(got), half_ulp)).clamp_min(0)


def test_gelu_bf16_forward_every_finite_value(gelu_table):
    """|gelu(u) - gelu_erf64(u)| <= 3e-5 + 2^-7 |ref| at every finite bf16 u, no NaN: the fit's documented 2.6e-5 (cvcl_common.h)
    plus room for the hardware rcp / exp2, and one bf16 ulp.  Measured on the MI355X: largest |err| / bound 0.612 at u = -3.125
    (|err| 3.16e-5 against 5.17e-5); the error that bf16 rounding cannot explain peaks at 2.45e-5 (u = -3.07812), inside the
    documented 2.6e-5; no element outside.  (The bound pins the fit, the saturation and the huge magnitudes; it does not pin the
    clamp's exact position: a clamp at v^2 = 16 moves the function by about 1e-5 on 4 < |u| < 6 only, which 3e-5 allows.)"""
    t = gelu_table
    got = t["y"].double()
    assert bool(torch.isfinite(got).all())
    err = (got - t["ref_y"]).abs()
    bound = 3e-5 + 2.0 ** -7 * t["ref_y"].abs()
    net = beyond_rounding(got, err)
    i = int(net.argmax())
    print(f"GELU bf16 forward: {worst(err, bound, t['u'])}; error beyond bf16 rounding peaks at {float(net[i]):.3e} (u = {float(t['u'][i]):.6g})")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} values outside the bound"


def test_gelu_bf16_backward_every_finite_value(gelu_table):
    """d_y = 1: |gelu'(u) - gelu'64(u)| <= 1e-6 + 2^-7 |ref| (Abramowitz-Stegun erf: 1.5e-7, 7.5e-8 on the CDF; fp32 evaluation
    2.7e-7 in total).  A random bf16 d_y: |got - d_y gelu'64(u)| <= |d_y| (1e-6 + 2^-7 |gelu'64|).  Measured on the MI355X:
    largest |err| / bound 0.497 (d_y = 1, u = 0.00244141) and 0.495 (random d_y, u = 0.0361328), both plain bf16 rounding; the
    error that bf16 rounding cannot explain peaks at 1.3e-8 (d_y = 1, u = -5.53125); no element outside either bound."""
    t = gelu_table
    d = t["d"].double()
    for name, got, ref, scale in (("d_y = 1", t["g"].double(), t["ref_g"], torch.ones_like(d)), ("random d_y", t["du"].double(), t["ref_g"] * d, d.abs())):
        assert bool(torch.isfinite(got).all())
        err = (got - ref).abs()
        bound = scale * 1e-6 + 2.0 ** -7 * ref.abs()
        net = beyond_rounding(got, err)
        i = int(net.argmax())
        print(f"GELU bf16 backward, {name}: {worst(err, bound, t['u'])}; error beyond bf16 rounding peaks at {float(net[i]):.3e} "
              f"(u = {float(t['u'][i]):.6g})")
        assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} values outside the bound"


def test_gelu_bf16_second_grid_stride_trip(H, dev, gelu_table):
    """The table tiled 258 times (16 842 240 elements, one more trip of the grid-stride loop than 8192 workgroups cover) gives the
    tiled output of the small call, forward and backward."""
    t = gelu_table
    lib, st = H.lib(), H.stream_ptr()
    n = t["u"].numel() * GELU_TILES
    assert n > 8192 * 256 * 8
    ud, dd = t["u"].to(dev).repeat(GELU_TILES), t["d"].to(dev).repeat(GELU_TILES)
    for d_y, small in ((None, t["y"]), (dd, t["du"])):
        y = torch.full((n,), NAN, dtype=BF, device=dev)
        H.check(lib.cvcl_gelu_bf16(H.ptr(ud), H.ptr(d_y), H.ptr(y), n, st), "cvcl_gelu_bf16")
        torch.cuda.synchronize()
        assert torch.equal(y, small.to(dev).repeat(GELU_TILES))


# ---- 5. attention at the limits of T -----------------------------------------------------------------------------------------------

def attn_case(H, dev, B, T, heads, q_gain):
    """cvcl_attention_train + cvcl_attention_bwd against float64 autograd of softmax(q k^T / 8) v on the same bf16 operands, both run
    twice.  -> (O max-abs / max|ref|, LSE max-abs, [dQ, dK, dV max-abs / max|ref|], [their cosines], the largest |logit|)."""
    g = torch.Generator().manual_seed(T * 13 + heads)
    D = heads * 64
    qkv = torch.randn(B, T, 3, heads, 64, generator=g) * 1.2
    qkv[:, :, 0] *= q_gain
    qkv = qkv.to(BF)
    d_o = torch.randn(B, T, D, generator=g).to(BF)
    q64 = qkv.double().requires_grad_(True)
    q, k, v = (q64[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    logits = q @ k.transpose(-1, -2) * 0.125
    ref = (torch.softmax(logits, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, T, D)
    ref.backward(d_o.double())
    ref, logits = ref.detach(), logits.detach()
    lse_ref = torch.logsumexp(logits, dim=-1) / math.log(2.0)
    lib, st = H.lib(), H.stream_ptr()
    qd, dod = qkv.to(dev).contiguous(), d_o.to(dev)
    runs = []
    for _ in range(2):
        out = torch.full((B, T, D), NAN, dtype=BF, device=dev)
        lse = torch.full((B, heads, T), NAN, device=dev)
        dq = torch.full((B, T, 3, heads, 64), NAN, dtype=BF, device=dev)
        H.check(lib.cvcl_attention_train(H.ptr(qd), H.ptr(out), H.ptr(lse), B, T, heads, 64, 0.125, st), "cvcl_attention_train")
        H.check(lib.cvcl_attention_bwd(H.ptr(qd), H.ptr(out), H.ptr(dod), H.ptr(lse), H.ptr(dq), B, T, heads, 64, 0.125, st),
                "cvcl_attention_bwd")
        torch.cuda.synchronize()
        runs.append((out.cpu(), lse.cpu(), dq.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    out, lse, dq = runs[0]
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dq.float()).all()
    e_o = float((out.double() - ref).abs().max() / ref.abs().max())
    e_l = float((lse.double() - lse_ref).abs().max())
    got, want = dq.double(), q64.grad
    rel = [float((got[:, :, i] - want[:, :, i]).abs().max() / want[:, :, i].abs().max()) for i in range(3)]
    cos = [float(torch.nn.functional.cosine_similarity(got[:, :, i].flatten(), want[:, :, i].flatten(), dim=0)) for i in range(3)]
    return e_o, e_l, rel, cos, float(logits.abs().max())


def show_attn(tag, e_o, e_l, rel, cos):
    print(f"attention bf16 {tag}: O {e_o:.2e}  LSE {e_l:.2e}  dQ/dK/dV max-rel " + " ".join(f"{r:.2e}" for r in rel)
          + "  1 - cosine " + " ".join(f"{1 - c:.1e}" for c in cos))


# T = 33: the smallest accepted, one key past a 32-tile; 64 and 65: either side of a tile boundary; 288: the largest accepted
@pytest.mark.parametrize("B,T,heads", [(1, 33, 1), (2, 64, 1), (1, 65, 3), (1, 288, 2)])
def test_attention_bf16_limits_of_T_vs_float64(H, dev, B, T, heads):
    """Bounds of test_attention_backward_vs_float64 (test_encoders_gpu.py): O and LSE < 2e-2, dQ / dK / dV max-rel < 3e-2 and
    cosine > 0.9995; bit-identical reruns."""
    e_o, e_l, rel, cos, _ = attn_case(H, dev, B, T, heads, 1.0)
    show_attn(f"B {B} T {T} heads {heads}", e_o, e_l, rel, cos)
    assert e_o < 2e-2 and e_l < 2e-2
    assert max(rel) < 3e-2 and min(cos) > 0.9995


def test_attention_bf16_near_one_hot_vs_float64(H, dev):
    """T = 197 with q scaled by 25: the logits span more than 80 (largest |logit| 199.6), the rows are near one-hot and the saved
    log-sum-exp carries the softmax.  Each bound is twice the error measured on the MI355X (the errors depend on the seed's few
    dominant keys); all of them are below the cap of four times the plain case's bounds (8e-2, 8e-2, 1.2e-1, 1 - cosine 2e-3).
    Measured: O 1.97e-3, LSE 2.07e-5, dQ / dK / dV max-rel 3.26e-3 / 5.12e-3 / 2.40e-3, 1 - cosine 1.6e-5 / 1.6e-5 / 1.6e-6."""
    e_o, e_l, rel, cos, span = attn_case(H, dev, 1, 197, 2, 25.0)
    show_attn(f"near one-hot, max |logit| {span:.1f}", e_o, e_l, rel, cos)
    assert span > 80
    assert e_o < 3.94e-3 and e_l < 4.14e-5
    for r, c, r_max, c_max in zip(rel, cos, (6.52e-3, 1.024e-2, 4.80e-3), (3.2e-5, 3.2e-5, 3.2e-6)):
        assert r < r_max and 1 - c < c_max, (rel, cos)


def test_attention_bf16_refusals_leave_outputs_untouched(H, dev):
    lib, st = H.lib(), H.stream_ptr()
    B, heads = 2, 4
    qkv = torch.zeros(B, 300, 3 * heads * 64, dtype=BF, device=dev)
    canary = torch.full((B * 300 * heads * 64 * 3,), 7.0, dtype=BF, device=dev)
    lse = torch.full((B * heads * 300,), 7.0, device=dev)
    p = H.ptr
    for hd, T in ((32, 197), (64, 32), (64, 289)):
        assert lib.cvcl_attention_train(p(qkv), p(canary), p(lse), B, T, heads, hd, 0.125, st) == EINVAL, (hd, T)
        assert lib.cvcl_attention_bwd(p(qkv), p(qkv), p(qkv), p(lse), p(canary), B, T, heads, hd, 0.125, st) == EINVAL, (hd, T)
    assert lib.cvcl_attention_train(None, p(canary), p(lse), B, 197, heads, 64, 0.125, st) == EINVAL
    assert lib.cvcl_attention_bwd(p(qkv), None, p(qkv), p(lse), p(canary), B, 197, heads, 64, 0.125, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all()) and bool((lse == 7.0).all())
