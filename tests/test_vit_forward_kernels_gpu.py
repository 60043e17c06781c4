"""GPU: the frozen ViT forward kernels that are not GEMMs (csrc/vit.hip and the two activation quantisers of csrc/gemm_fp8.hip), one C
entry at a time, against float64 (or, where a kernel only copies, adds once or rounds, the same IEEE operation) on the CPU computed
from exactly the values the kernel receives.  Every entry picks one of several kernels from the dtype, the shape, the row count and
the pointer alignment; the cases below reach every one of those routes: patch gather and token assembly (16-byte and scalar paths,
second grid-stride trips), the seven LayerNorm kernels, the row statistics, the generic attention with a key padding mask, the MX
attention epilogue at the two-pass token counts, and every instantiation of the per-row e4m3 and the MX block quantisers.  Every
output starts as NaN (or a canary byte), every kernel runs twice and must repeat itself bit for bit, a refused call returns EINVAL
and leaves its outputs untouched, and each case prints the error it measured."""
import pytest
import torch

from conftest import maxrel
from test_gemm_gpu import _mx_quant_ref, _mx_tile_scales, _quant_rows_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
NAN = float("nan")
EINVAL = -1
FWD = 2e-5                                             # fp32 forward values, maxrel (tests/test_text_head_kernels_gpu.py)
CAP = 8192 * 256                                       # threads of a capped grid-stride launch (cvcl_grid(n, 256, 8192))


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    _hip.load()
    return _hip


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def twice(make, launch):
    """Fresh outputs from make(), launch(*outputs), twice: the two runs must agree bit for bit (NaN canaries included).
    -> the first run's outputs on the CPU."""
    runs = []
    for _ in range(2):
        outs = make()
        launch(*outs)
        torch.cuda.synchronize()
        runs.append([o.cpu() for o in outs])
    assert all(same_bits(a, b) for a, b in zip(*runs))
    return runs[0]


def off_by_one(t, dev):
    """A device copy of t that starts one element past an allocation's (16-byte aligned) base."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def worst_ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


# ---- 1. patch gather ---------------------------------------------------------------------------------------------------------------

def im2col_ref(x, p, Kpad):
    """cols[b np + py gw + px][c p^2 + ky p + kx] = x[b][c][py p + ky][px p + kx], zero from 3 p^2 to Kpad."""
    B, _, Hh, W = x.shape
    u = x.unfold(2, p, p).unfold(3, p, p)                                  # [B, 3, gh, gw, ky, kx]
    out = torch.zeros(B * (Hh // p) * (W // p), Kpad)
    out[:, :3 * p * p] = u.permute(0, 2, 3, 1, 4, 5).reshape(out.shape[0], 3 * p * p)
    return out


def im2col_case(H, dev, bf16, B, Hh, W, p, Kpad, misaligned=False):
    torch.manual_seed(p * 1000 + Kpad + B)
    n = B * 3 * Hh * W
    x = torch.randn(B, 3, Hh, W) if bf16 else (torch.arange(n, dtype=torch.float32) * 0.25 - 1000.0).reshape(B, 3, Hh, W)
    ref = im2col_ref(x, p, Kpad)
    ref = ref.bfloat16() if bf16 else ref
    xd = off_by_one(x, dev) if misaligned else x.to(dev)
    assert (xd.data_ptr() % 16 != 0) == misaligned
    lib, st = H.lib(), H.stream_ptr()
    cols, = twice(lambda: [torch.full(ref.shape, NAN, dtype=ref.dtype, device=dev)],
                  lambda c: H.check(lib.cvcl_im2col_patches(H.BF16 if bf16 else H.F32, H.ptr(xd), H.ptr(c), B, Hh, W, p, Kpad, st),
                                    "cvcl_im2col_patches"))
    print(f"im2col {'bf16' if bf16 else 'fp32'} B {B} {Hh}x{W} patch {p} Kpad {Kpad} misaligned {misaligned}: "
          f"{int((cols.float() != ref.float()).sum())} of {ref.numel()} elements differ")
    assert torch.equal(cols, ref)


# (bf16, patch, Kpad, misaligned); the image is 2 x 3 patches (H = 2 p, W = 3 p), B = 3
IM2COL_CASES = [(False, 16, 768, False), (False, 14, 592, False), (True, 16, 768, False), (True, 16, 784, False),
                (True, 8, 192, False), (True, 14, 592, False), (True, 16, 768, True)]


@pytest.mark.parametrize("bf16,p,Kpad,misaligned", IM2COL_CASES)
def test_im2col_patches_exact(H, dev, bf16, p, Kpad, misaligned):
    """cvcl_im2col_patches copies (fp32) or rounds to nearest even (bf16): torch.equal against unfold on the CPU, the columns from
    3 p^2 to Kpad written as zeros over the NaN fill.  fp32 (patch 16; patch 14 with K = 588 padded to 592): im2col_patches_kernel
    <float>.  bf16 patch 16 / Kpad 768, Kpad 784 (two zero chunks per row) and patch 8: im2col_patches8_kernel, as patch % 8 == 0,
    Kpad % 8 == 0, W % 4 == 0 and both pointers sit on 16 bytes.  bf16 patch 14 (patch % 8 != 0) and patch 16 with x one float past
    a 16-byte boundary: im2col_patches_kernel<bf16>.  The image is not square (2 x 3 patches), so gh / gw and ky / kx cannot be
    swapped; fp32 values are all distinct (an arithmetic sequence), bf16 values random."""
    im2col_case(H, dev, bf16, 3, 2 * p, 3 * p, p, Kpad, misaligned)


@pytest.mark.parametrize("B,p,Kpad", [(16, 14, 592), (112, 16, 768)])
def test_im2col_patches_second_grid_stride_trip(H, dev, B, p, Kpad):
    """224 x 224 images, more work items than the 8192 x 256 threads of the capped launch: B = 16 at patch 14 is 2 424 832 elements
    of the scalar bf16 kernel; B = 112 at patch 16 is 2 107 392 chunks of the 16-byte kernel (B = 111 is 2 088 576: one trip)."""
    items = B * (224 // p) ** 2 * Kpad // (8 if p % 8 == 0 else 1)
    assert CAP < items < 2 * CAP
    im2col_case(H, dev, True, B, 224, 224, p, Kpad)


def test_im2col_patches_refusals_leave_output_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    x = torch.zeros(3, 3, 32, 48, device=dev)
    cols = torch.full((3 * 6 * 800,), 7.0, device=dev)                    # read as fp32 or bf16: large enough for both
    for dt in (H.F32, H.BF16):
        assert lib.cvcl_im2col_patches(dt, p(x), p(cols), 3, 30, 48, 16, 768, st) == EINVAL       # H % patch
        assert lib.cvcl_im2col_patches(dt, p(x), p(cols), 3, 32, 48, 16, 760, st) == EINVAL       # Kpad < 3 p^2
        assert lib.cvcl_im2col_patches(dt, None, p(cols), 3, 32, 48, 16, 768, st) == EINVAL
        assert lib.cvcl_im2col_patches(dt, p(x), None, 3, 32, 48, 16, 768, st) == EINVAL
    for dt in (2, 3):
        assert lib.cvcl_im2col_patches(dt, p(x), p(cols), 3, 32, 48, 16, 768, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((cols == 7.0).all())


# ---- 2. token assembly -------------------------------------------------------------------------------------------------------------

# (bf16, D, misaligned tok)
ASSEMBLE_ROUTES = [(False, 100, False), (True, 768, False), (True, 8, False), (True, 100, False), (True, 768, True)]


@pytest.mark.parametrize("T", [2, 5, 197])
@pytest.mark.parametrize("bf16,D,misaligned", ASSEMBLE_ROUTES)
def test_vit_assemble_tokens_exact(H, dev, bf16, D, misaligned, T):
    """cvcl_vit_assemble_tokens: h[b][0] = cls + pos[0], h[b][t] = tok[b][t - 1] + pos[t], one IEEE fp32 addition (then one rounding
    to bf16): torch.equal against the same addition on the CPU.  fp32 D = 100: vit_assemble_kernel<float>; bf16 D = 768 and D = 8
    (one chunk per row): vit_assemble8_kernel; bf16 D = 100 (D % 8 != 0) and D = 768 with tok one element past a 16-byte boundary:
    vit_assemble_kernel<bf16>.  T = 2 is the smallest accepted; B = 3; cls, pos and tok are random and all different."""
    torch.manual_seed(D * 10 + T + int(bf16))
    B = 3
    tok = torch.randn(B, T - 1, D)
    tok = tok.bfloat16() if bf16 else tok
    cls, pos = torch.randn(D), torch.randn(T, D)
    ref = torch.cat([cls.expand(B, 1, D), tok.float()], 1) + pos
    ref = ref.bfloat16() if bf16 else ref
    tokd = off_by_one(tok, dev) if misaligned else tok.to(dev)
    assert (tokd.data_ptr() % 16 != 0) == misaligned
    clsd, posd = cls.to(dev), pos.to(dev)
    lib, st = H.lib(), H.stream_ptr()
    h, = twice(lambda: [torch.full((B, T, D), NAN, dtype=ref.dtype, device=dev)],
               lambda o: H.check(lib.cvcl_vit_assemble_tokens(H.BF16 if bf16 else H.F32, H.ptr(tokd), H.ptr(clsd), H.ptr(posd), H.ptr(o),
                                                              B, T, D, st), "cvcl_vit_assemble_tokens"))
    print(f"assemble {'bf16' if bf16 else 'fp32'} T {T} D {D} misaligned {misaligned}: "
          f"{int((h.float() != ref.float()).sum())} of {ref.numel()} elements differ")
    assert torch.equal(h, ref)


def test_vit_assemble_tokens_refusals_leave_output_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    tok, cls, pos = torch.zeros(3, 4, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(5, 8, device=dev)
    h = torch.full((3 * 5 * 8,), 7.0, device=dev)
    for dt in (H.F32, H.BF16):
        assert lib.cvcl_vit_assemble_tokens(dt, p(tok), p(cls), p(pos), p(h), 3, 1, 8, st) == EINVAL          # T = 1: no patch token
        assert lib.cvcl_vit_assemble_tokens(dt, None, p(cls), p(pos), p(h), 3, 5, 8, st) == EINVAL
        assert lib.cvcl_vit_assemble_tokens(dt, p(tok), None, p(pos), p(h), 3, 5, 8, st) == EINVAL
        assert lib.cvcl_vit_assemble_tokens(dt, p(tok), p(cls), None, p(h), 3, 5, 8, st) == EINVAL
        assert lib.cvcl_vit_assemble_tokens(dt, p(tok), p(cls), p(pos), None, 3, 5, 8, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((h == 7.0).all())


# ---- 3. LayerNorm ------------------------------------------------------------------------------------------------------------------

def ln_ref(x, gamma, beta, eps):
    """float64 LayerNorm of rows x [rows, D]: -> (y, s); s = rstd |x - mean| |gamma| + |beta|, the magnitudes of the terms of y."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    xc = x - x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    return xc * rstd * gamma + beta, rstd * xc.abs() * gamma.abs() + beta.abs()


def ln_inputs(rows, D, xs, bf16):
    torch.manual_seed(rows * 7 + D)
    x = torch.randn(rows, xs) * 2 + 0.5                # a non-zero mean: the centring matters
    return (x.bfloat16() if bf16 else x), torch.rand(D) + 0.5, torch.randn(D)


def ln_run(H, dev, xd, xs, gamma, beta, eps, bf16, y_f32, rows, D):
    """cvcl_layernorm into a y three rows longer than asked for: -> y [rows, D] on the CPU; the three rows beyond stay NaN."""
    lib, st = H.lib(), H.stream_ptr()
    gd, bd = gamma.to(dev), beta.to(dev)
    y, = twice(lambda: [torch.full((rows + 3, D), NAN, dtype=torch.float32 if y_f32 else BF, device=dev)],
               lambda o: H.check(lib.cvcl_layernorm(H.BF16 if bf16 else H.F32, H.ptr(xd), xs, H.ptr(gd), H.ptr(bd), eps, H.ptr(o),
                                                    int(y_f32), rows, D, st), "cvcl_layernorm"))
    assert bool(torch.isnan(y[rows:].float()).all()), "rows beyond `rows` were written"
    assert bool(torch.isfinite(y[:rows].float()).all())
    return y[:rows]


def ln_case(H, dev, bf16, y_f32, rows, D, strided=False, misaligned=False, eps=1e-6):
    xs = 3 * D if strided else D                       # strided rows: the cls rows of [B][T][D]
    x, gamma, beta = ln_inputs(rows, D, xs, bf16)
    ref, s = ln_ref(x[:, :D], gamma, beta, eps)
    xd = off_by_one(x, dev) if misaligned else x.to(dev)
    y = ln_run(H, dev, xd, xs, gamma, beta, eps, bf16, y_f32, rows, D)
    tag = f"LN {'bf16' if bf16 else 'fp32'} -> {'fp32' if y_f32 else 'bf16'} rows {rows} D {D} strided {strided} misaligned {misaligned} eps {eps:g}"
    if y_f32:
        e = maxrel(y, ref)
        print(f"{tag}: maxrel {e:.2e}")
        assert e < FWD
    else:
        err = (y.double() - ref).abs()
        bound = 2.0 ** -7 * ref.abs() + 2.0 ** -18 * s
        print(f"{tag}: max err/bound {worst_ratio(err, bound):.3f}")
        assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements outside the bound"


@pytest.mark.parametrize("rows,D,strided,eps", [(5, 100, False, 1e-6), (4, 8, False, 1e-6), (1001, 512, False, 1e-6),
                                                (7, 768, True, 1e-6), (5, 100, False, 1e-5)])
def test_layernorm_f32_vs_float64(H, dev, rows, D, strided, eps):
    """CVCL_F32: layernorm_kernel<float, float>, one wave per row, whatever the shape -- D = 100 (a ragged second trip of the lane
    loop), D = 8 (56 idle lanes), 1001 rows (a last workgroup with one row), 7 rows at stride 3 D.  maxrel < 2e-5 against float64.
    Measured on the MI355X: at most 1.2e-7."""
    ln_case(H, dev, False, True, rows, D, strided=strided, eps=eps)


@pytest.mark.parametrize("rows,D,eps", [(4099, 768, 1e-6), (4099, 384, 1e-6), (4096, 8, 1e-6), (4100, 760, 1e-6), (4099, 384, 1e-5)])
def test_layernorm_bf16_row32_vs_float64(H, dev, rows, D, eps):
    """bf16 -> bf16, D <= 768 and rows >= 4096: 32 lanes per row, 3 chunks of 8 per lane.  D = 768: layernorm_bf16_row32_kernel
    <bf16, 3, true> (every chunk exists); D = 384 (lanes 16 to 31 hold one chunk, none a third), D = 8 (one lane holds the row) and
    D = 760 (95 chunks: lane 31 alone lacks its third): <bf16, 3, false>.  4099 and 4100 rows leave a last workgroup with 3 and 4 of
    its 8 rows.  Every element: |got - ref| <= 2^-7 |ref| + 2^-18 s, s = rstd |x - mean| |gamma| + |beta| (2^-8 is the worst-case
    rounding to bf16; the second 2^-8 and the fp32 floor leave room for a different fp32 summation order that flips a rounding).
    Measured on the MI355X: at most 0.498 of the bound on either instantiation (plain bf16 rounding)."""
    ln_case(H, dev, True, False, rows, D, eps=eps)


@pytest.mark.parametrize("y_f32,rows,D,strided", [(False, 1001, 768, False), (False, 4100, 1024, False), (False, 300, 2048, False),
                                                  (False, 64, 776, False), (True, 5, 768, True), (True, 300, 2048, False)])
def test_layernorm_bf16_vec_vs_float64(H, dev, y_f32, rows, D, strided):
    """bf16 rows with D % 8 == 0, D <= 2048, everything on 16 bytes, outside the row32 window: one wave per row, up to 4 chunks per
    lane.  -> bf16, layernorm_bf16_vec_kernel<bf16>: (1001, 768) has rows < 4096, (4100, 1024) has D > 768, (300, 2048) fills all
    4 chunks of every lane, (64, 776) leaves lane 33 and up with one chunk.  -> fp32, layernorm_bf16_vec_kernel<float>: the final
    norm's call (5 cls rows at stride 3 D) and (300, 2048).  Bounds: bf16 output as test_layernorm_bf16_row32_vs_float64, fp32
    output maxrel < 2e-5.  Measured on the MI355X: bf16 at most 0.498 of the bound, fp32 at most 1.2e-7."""
    ln_case(H, dev, True, y_f32, rows, D, strided=strided)


@pytest.mark.parametrize("y_f32", [False, True])
@pytest.mark.parametrize("rows,D,misaligned", [(17, 100, False), (3, 2056, False), (9, 768, True)])
def test_layernorm_bf16_scalar_vs_float64(H, dev, rows, D, misaligned, y_f32):
    """bf16 rows the 16-byte kernels cannot take -- D % 8 != 0 (100), D > 2048 (2056), x one element past a 16-byte boundary (768):
    layernorm_kernel<bf16, bf16> and layernorm_kernel<bf16, float>.  Bounds as the vec kernels'.  Measured on the MI355X: bf16 at most
    0.498 of the bound, fp32 at most 1.3e-7."""
    ln_case(H, dev, True, y_f32, rows, D, misaligned=misaligned)


def test_layernorm_bf16_row32_and_vec_agree(H, dev):
    """A cross-route line: the first 1001 rows of the (4099, 768) input through the vec kernel (rows < 4096) against the same rows of
    the row32 kernel's output, within the bound of test_layernorm_bf16_row32_vs_float64.  Measured on the MI355X: 10 of the 768 768
    elements differ (a flipped bf16 rounding each), by 0.883 of the bound at most."""
    x, gamma, beta = ln_inputs(4099, 768, 768, True)
    ref, s = ln_ref(x[:1001], gamma, beta, 1e-6)
    a = ln_run(H, dev, x.to(dev), 768, gamma, beta, 1e-6, True, False, 4099, 768)[:1001]
    b = ln_run(H, dev, x[:1001].to(dev), 768, gamma, beta, 1e-6, True, False, 1001, 768)
    diff = (a.double() - b.double()).abs()
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -18 * s
    print(f"LN bf16 row32 vs vec, 1001 x 768: max diff/bound {worst_ratio(diff, bound):.3f}, {int((diff != 0).sum())} of {diff.numel()} differ")
    assert bool((diff <= bound).all())


def test_layernorm_refusals_leave_output_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    x = torch.zeros(10 * 768, device=dev)
    g, b = torch.ones(768, device=dev), torch.zeros(768, device=dev)
    y = torch.full((10 * 768,), 7.0, device=dev)
    for dt in (H.F32, H.BF16):
        for yf in (0, 1):
            assert lib.cvcl_layernorm(dt, p(x), 760, p(g), p(b), 1e-6, p(y), yf, 5, 768, st) == EINVAL     # x_row_stride < D
            assert lib.cvcl_layernorm(dt, None, 768, p(g), p(b), 1e-6, p(y), yf, 5, 768, st) == EINVAL
            assert lib.cvcl_layernorm(dt, p(x), 768, None, p(b), 1e-6, p(y), yf, 5, 768, st) == EINVAL
            assert lib.cvcl_layernorm(dt, p(x), 768, p(g), None, 1e-6, p(y), yf, 5, 768, st) == EINVAL
            assert lib.cvcl_layernorm(dt, p(x), 768, p(g), p(b), 1e-6, None, yf, 5, 768, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---- 4. row statistics -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,D,strided", [(5, 768, True), (4096, 8, False)])
def test_row_stats_strided_and_narrow_vs_float64(H, dev, rows, D, strided):
    """cvcl_row_stats, row_stats_bf16_kernel<3>: 5 cls rows at stride 3 D, and 4096 rows of one chunk each (31 idle lanes per row).
    (rstd, -mean rstd) against float64 with the tolerance of tests/test_lnfold_gpu.py: 2e-6 relative on rstd, 2e-6 (max |mean rstd|
    + 1) on the second.  Measured on the MI355X: at most 1.7e-7 and 3.3e-7."""
    xs = 3 * D if strided else D
    x, _, _ = ln_inputs(rows, D, xs, True)
    xd = x.to(dev)
    lib, st = H.lib(), H.stream_ptr()
    out, = twice(lambda: [torch.full((rows + 3, 2), NAN, device=dev)],
                 lambda o: H.check(lib.cvcl_row_stats(H.BF16, H.ptr(xd), xs, H.ptr(o), rows, D, 1e-6, st), "cvcl_row_stats"))
    assert bool(torch.isnan(out[rows:]).all())
    x64 = x[:, :D].double()
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    got = out[:rows].double()
    e0 = float(((got[:, 0] - rstd).abs() / rstd).max())
    e1 = float((got[:, 1] + mean * rstd).abs().max())
    print(f"row_stats rows {rows} D {D} strided {strided}: rstd rel {e0:.2e}  -mean rstd abs {e1:.2e}")
    assert e0 < 2e-6
    assert e1 < 2e-6 * float((mean * rstd).abs().max() + 1)


def test_row_stats_refusals_leave_output_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    x = torch.zeros(4, 1032, dtype=BF, device=dev)
    out = torch.full((8,), 7.0, device=dev)
    assert lib.cvcl_row_stats(H.BF16, p(x), 1032, p(out), 4, 1032, 1e-6, st) == EINVAL                       # D > 1024
    assert lib.cvcl_row_stats(H.BF16, p(x), 1032, p(out), 4, 100, 1e-6, st) == EINVAL                        # D % 8
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 5. generic attention with a key padding mask ----------------------------------------------------------------------------------

def key_tokens(B, T, shift, g):
    """int64 tokens [B, T], 0 = padding.  Sequence b takes mask kind (b + shift) % 4: padding at the end (as lengths give), zeros in
    the middle, only key 0 valid, no padding.  Every sequence keeps at least one valid key."""
    tok = torch.randint(1, 1000, (B, T), generator=g)
    for b in range(B):
        kind = (b + shift) % 4
        if kind == 0:
            tok[b, T - max(1, T // 3):] = 0
        elif kind == 1:
            tok[b, T // 3:T // 3 + max(1, T // 4)] = 0
        elif kind == 2:
            tok[b, 1:] = 0
    assert bool((tok != 0).any(1).all())
    return tok


def masked_attention_case(H, dev, bf16, B, T, heads, hd, shift):
    g = torch.Generator().manual_seed(T * 31 + hd + (shift if shift is not None else 7))
    qkv = torch.randn(B, T, 3, heads, hd, generator=g) * 1.2
    qkv = qkv.bfloat16() if bf16 else qkv
    tok = key_tokens(B, T, shift, g) if shift is not None else None
    scale = float(torch.tensor(hd ** -0.5, dtype=torch.float32))
    q, k, v = (qkv.double()[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    logits = q @ k.transpose(-1, -2) * scale
    if tok is not None:
        logits = logits.masked_fill((tok == 0)[:, None, None, :], float("-inf"))
    p = torch.softmax(logits, dim=-1)
    if bf16:
        p = p.to(BF).double()                          # the kernel rounds P to the storage type before P V
    D = heads * hd
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B, T, D)
    floor = (p @ v.abs()).permute(0, 2, 1, 3).reshape(B, T, D)
    qd, tokd = qkv.to(dev).contiguous(), tok.to(dev) if tok is not None else None
    lib, st = H.lib(), H.stream_ptr()
    out, = twice(lambda: [torch.full((B, T, D), NAN, dtype=qkv.dtype, device=dev)],
                 lambda o: H.check(lib.cvcl_attention(H.BF16 if bf16 else H.F32, H.ptr(qd), H.ptr(tokd), H.ptr(o), B, T, heads, hd, scale, st),
                                   "cvcl_attention"))
    assert bool(torch.isfinite(out.float()).all())
    tag = f"attention {'bf16' if bf16 else 'fp32'} B {B} T {T} heads {heads} hd {hd} mask {'none' if shift is None else shift}"
    if bf16:
        err = (out.double() - ref).abs()
        bound = 2.0 ** -7 * ref.abs() + 2.0 ** -8 * floor
        print(f"{tag}: max err/bound {worst_ratio(err, bound):.3f}")
        assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements outside the bound"
    else:
        e = maxrel(out, ref)
        print(f"{tag}: maxrel {e:.2e}")
        assert e < FWD


@pytest.mark.parametrize("shift", [0, 1, 2, 3, None])
@pytest.mark.parametrize("B,T,heads,hd", [(3, 5, 2, 24), (2, 25, 8, 64), (1, 70, 3, 128), (1, 3, 1, 8)])
def test_attention_f32_key_padding_mask_vs_float64(H, dev, B, T, heads, hd, shift):
    """cvcl_attention, CVCL_F32: attention_valu_kernel<float>, one wave per (b, head, query), against float64 softmax(q k^T scale +
    mask) v with -inf where key_tok == 0.  (2, 25, 8, 64) is the text transformer's own shape; (1, 70, 3, 128) gives lanes 0 to 5 two
    keys each and the output loop two trips; (1, 3, 1, 8) leaves the only workgroup with an idle wave.  `shift` rotates the four mask
    kinds (end padding, zeros in the middle, only key 0 valid, none) over the sequences, so every case sees every kind; None passes
    key_tok = NULL.  maxrel < 2e-5.  Measured on the MI355X: at most 9.8e-7."""
    masked_attention_case(H, dev, False, B, T, heads, hd, shift)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("B,T,heads,hd", [(2, 70, 2, 64), (2, 9, 2, 24)])
def test_attention_bf16_key_padding_mask_vs_float64(H, dev, B, T, heads, hd, shift):
    """cvcl_attention, CVCL_BF16 with a mask: attention_valu_kernel<bf16> -- at (2, 70, 2, 64) only the mask keeps the call from the
    MFMA kernel (head_dim 64, 32 < T <= 288).  The reference rounds P to bf16 before P V, as the kernel does; every element:
    |got - ref| <= 2^-7 |ref| + 2^-8 sum_j p_j |v_jd| (the second term covers every P flipping its bf16 rounding because the fp32
    softmax differs from float64).  Measured on the MI355X: at most 0.304 of the bound (the unmasked (2, 9, 2, 24) call below included)."""
    masked_attention_case(H, dev, True, B, T, heads, hd, shift)


def test_attention_bf16_small_without_mask_vs_float64(H, dev):
    """(2, 9, 2, 24) with key_tok = NULL: T <= 32 and head_dim != 64 keep the bf16 call on the generic kernel."""
    masked_attention_case(H, dev, True, 2, 9, 2, 24, None)


def test_attention_refusals_leave_output_untouched(H, dev):
    """head_dim 129, and T = 4033 at head_dim 64: 4 waves x (64 + 4033) floats = 65 552 bytes of LDS > 64 KiB (T = 4032 fits)."""
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    T = 4096 - 64 + 1
    assert 4 * (64 + T) * 4 > 65536 >= 4 * (64 + T - 1) * 4
    qkv = torch.zeros(T * 3 * 129, device=dev)                            # large enough for both refused shapes, fp32 or bf16
    tok = torch.ones(T, dtype=torch.int64, device=dev)
    out = torch.full((T * 129,), 7.0, device=dev)
    for dt in (H.F32, H.BF16):
        for kt in (None, p(tok)):
            assert lib.cvcl_attention(dt, p(qkv), kt, p(out), 1, 5, 1, 129, 0.125, st) == EINVAL
            assert lib.cvcl_attention(dt, p(qkv), kt, p(out), 1, T, 1, 64, 0.125, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 6. MX attention epilogue at the remaining token counts ------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,heads,q_gain", [(1, 257, 2, 1.0), (1, 257, 2, 0.1), (1, 288, 2, 1.0), (2, 33, 4, 1.0), (3, 64, 2, 1.0)])
def test_attention_mx_output_matches_block_quantiser_other_T(H, dev, B, T, heads, q_gain):
    """cvcl_attention_mx = cvcl_attention's bf16 output pushed through the MX block quantiser, bit for bit (bytes and tiled scales),
    as test_attention_mx_output_matches_block_quantiser (test_encoders_gpu.py) has it at T = 197 and 50.  T = 257 and 288 have nine
    32-key tiles: attention_mfma_kernel<true, 9> against <false, 9>, the two-pass form (257 leaves 31 padded keys in the last tile,
    288 none); T = 33 (one key past a tile) and 64 run <true, 0> against <false, 0>.  Both sides share the softmax, so the bf16
    output is also held to float64 with the bound of test_attention_bf16_limits_of_T_vs_float64, max-abs < 2e-2 max |ref|; at q_gain
    0.1 the softmax is nearly uniform and the 31 padded keys of T = 257, if they were counted, would carry a ninth of the weight.
    Measured on the MI355X: at most 3.8e-3; no byte and no scale differs."""
    g = torch.Generator().manual_seed(T + heads)
    D = heads * 64
    qkv = torch.randn(B, T, 3, heads, 64, generator=g) * 1.5
    qkv[:, :, 0] *= q_gain
    qkv = qkv.bfloat16()
    q, k, v = (qkv.double()[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, T, D)
    qd = qkv.to(dev).contiguous()
    lib, st = H.lib(), H.stream_ptr()
    out, = twice(lambda: [torch.full((B, T, D), NAN, dtype=BF, device=dev)],
                 lambda o: H.check(lib.cvcl_attention(H.BF16, H.ptr(qd), None, H.ptr(o), B, T, heads, 64, 0.125, st), "cvcl_attention"))
    o8, obs = twice(lambda: [torch.full((B * T, D), 0xAA, dtype=torch.uint8, device=dev),
                             torch.full((D // 128, B * T, 4), 0xAA, dtype=torch.uint8, device=dev)],
                    lambda a, b: H.check(lib.cvcl_attention_mx(H.ptr(qd), H.ptr(a), H.ptr(b), B, T, heads, 64, 0.125, st), "cvcl_attention_mx"))
    e = float((out.double() - ref).abs().max() / ref.abs().max())
    q_ref, e_ref, _ = _mx_quant_ref(out.float().reshape(B * T, D))
    print(f"attention_mx B {B} T {T} heads {heads} q_gain {q_gain}: bf16 output max-abs / max|ref| {e:.2e}; "
          f"{int((o8 != q_ref.view(torch.uint8)).sum())} bytes and {int((obs != _mx_tile_scales(e_ref)).sum())} scales differ")
    assert e < 2e-2
    assert torch.equal(obs, _mx_tile_scales(e_ref))
    assert torch.equal(o8, q_ref.view(torch.uint8))


def test_attention_mx_refusals_leave_outputs_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    qkv = torch.zeros(2 * 300 * 3 * 4 * 64, dtype=BF, device=dev)
    o8 = torch.full((2 * 300 * 4 * 64,), 7, dtype=torch.uint8, device=dev)
    obs = torch.full((2 * 2 * 300 * 4,), 7, dtype=torch.uint8, device=dev)
    for T, heads, hd in ((197, 3, 64), (32, 4, 64), (289, 4, 64), (197, 4, 32)):
        assert lib.cvcl_attention_mx(p(qkv), p(o8), p(obs), 2, T, heads, hd, 0.125, st) == EINVAL, (T, heads, hd)
    assert lib.cvcl_attention_mx(None, p(o8), p(obs), 2, 197, 4, 64, 0.125, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((o8 == 7).all()) and bool((obs == 7).all())


# ---- 7. per-row e4m3 quantiser -----------------------------------------------------------------------------------------------------

def quant_rows_input(rows, K, xs, bf16):
    """randn * 1.7 rows [rows, xs] with four planted rows: all zeros (scale 1, bytes 0); amax exactly -448 * 2^-3 (scale 2^-3, byte
    0xFE); one element 1e4 over a row of order 1 (subnormal and zero codes); one repeated value (every byte 0x7E).  fp32 cases of
    300 rows or more hold bf16-rounded values (test_quant_rows_fp8_bit_identical_to_emulation says why)."""
    torch.manual_seed(K * 3 + rows)
    x = torch.randn(rows, xs) * 1.7
    x[0] = 0.0
    x[1, K // 2] = -56.0
    x[2, K - 1] = 1e4
    x[3] = 0.3
    if rows >= 300 and not bf16:
        x = x.bfloat16().float()                       # fp32 storage of 8-bit significands: y / s meets e4m3 ties as often as bf16 rows do
    return x.bfloat16() if bf16 else x


def quant_rows_run(H, dev, xd, xs, gamma, beta, bf16, rows, K):
    """cvcl_quant_rows_fp8 into outputs three rows longer than asked for: -> (bytes [rows, K], scale [rows]) on the CPU."""
    lib, st = H.lib(), H.stream_ptr()
    gd, bd = (gamma.to(dev), beta.to(dev)) if gamma is not None else (None, None)
    q, s = twice(lambda: [torch.full((rows + 3, K), 0xAA, dtype=torch.uint8, device=dev), torch.full((rows + 3,), NAN, device=dev)],
                 lambda a, b: H.check(lib.cvcl_quant_rows_fp8(H.BF16 if bf16 else H.F32, H.ptr(xd), xs, H.ptr(gd), H.ptr(bd), 1e-6,
                                                              H.ptr(a), H.ptr(b), rows, K, st), "cvcl_quant_rows_fp8"))
    assert bool((q[rows:] == 0xAA).all()) and bool(torch.isnan(s[rows:]).all()), "rows beyond `rows` were written"
    return q[:rows], s[:rows]


# (bf16, rows, K, strided)
QUANT_CASES = ([(False, 37, K, False) for K in (8, 200, 1024, 1032, 4096)] + [(True, 1000, 768, False)]
               + [(True, 37, K, False) for K in (8, 384, 760, 776, 1024, 1032, 3072, 4096)]
               + [(False, 37, 200, True), (True, 37, 384, True), (True, 37, 3072, True)]
               + [(False, 1000, 1024, False), (False, 300, 4096, False), (True, 1000, 760, False)])


@pytest.mark.parametrize("bf16,rows,K,strided", QUANT_CASES)
def test_quant_rows_fp8_bit_identical_to_emulation(H, dev, bf16, rows, K, strided):
    """cvcl_quant_rows_fp8 without LayerNorm: scales and e4m3 bytes bit-identical to _quant_rows_ref (amax / 448, RN(y / s),
    torch.float8_e4m3fn).  Instantiations <SRC_F32, LPR, NCH, EXACT> (the six the entry has): fp32 K <= 1024 (8, 200, 1024):
    <true, 32, 4, false>; fp32 K > 1024 (1032, 4096): <true, 64, 8, false>; bf16 K == 768: <false, 32, 3, true>; bf16 K < 768
    (8, 384, 760): <false, 32, 3, false>; bf16 768 < K <= 1024 (776, 1024): <false, 32, 4, false>; bf16 K > 1024 (1032, 3072,
    4096): <false, 64, 8, false>.  37 rows leave a tail for both 8 and 4 rows per workgroup; the strided cases read rows at stride
    K + 8.  Planted rows: quant_rows_input.
    The kernel forms RN(y / s) from RN(1 / s) by a quotient refinement; RN(y RN(1 / s)) alone differs from it where y / s sits on
    an e4m3 tie, which rows of 8-bit significands do in about 0.05 % of their elements and random fp32 rows never: 375 of the
    768 000 elements of the (1000, 768) case (counted on the CPU), none in the 37-row cases below K = 776.  So the three
    instantiations that (1000, 768) and the wide bf16 cases do not cover get a case of their own with enough such elements:
    fp32 storage of bf16-rounded values at (1000, 1024) and (300, 4096) (477 and 968 elements), bf16 at (1000, 760) (380)."""
    xs = K + 8 if strided else K
    x = quant_rows_input(rows, K, xs, bf16)
    q_ref, s_ref = _quant_rows_ref(x[:, :K].float())
    assert float(s_ref[0]) == 1.0 and float(s_ref[1]) == 0.125 and int(q_ref.view(torch.uint8)[1, K // 2]) == 0xFE
    q, s = quant_rows_run(H, dev, x.to(dev), xs, None, None, bf16, rows, K)
    print(f"quant_rows_fp8 {'bf16' if bf16 else 'fp32'} rows {rows} K {K} strided {strided}: {int((s != s_ref).sum())} scales and "
          f"{int((q != q_ref.view(torch.uint8)).sum())} of {q.numel()} bytes differ")
    assert torch.equal(s, s_ref)
    assert torch.equal(q, q_ref.view(torch.uint8))


def e4m3_code(q):
    """e4m3 bytes -> signed code numbers (adjacent representable values differ by one; +0 and -0 are both 0)."""
    q = q.int()
    return (q & 0x7F) * (1 - 2 * (q >> 7))


@pytest.mark.parametrize("bf16,K", [(False, 768), (True, 768), (True, 384), (True, 1024), (True, 3072)])
def test_quant_rows_fp8_with_layernorm_vs_float64(H, dev, bf16, K):
    """The fused mode the fp8 ViT uses (ln_gamma, ln_beta), one case per instantiation that model shapes reach.  With y the float64
    LayerNorm of the input, s the scale the kernel wrote, t = y / s and q the dequantised byte: |s - max |y| / 448| <= 2e-6 s, and
    per element |q - t| <= max(2^-4 |t|, 2^-10) + 448 * 2^-20 -- half an e4m3 step at |t| (three mantissa bits; a subnormal step of
    2^-9) plus the fp32 LayerNorm's rounding carried to the top of the range: a byte one code away from the correctly rounded one is
    allowed only inside that margin.  Measured on the MI355X: scale at most 1.3e-7 s, |q - t| at most 0.941 of the bound
    (16 / 17: half a step at the bottom of a binade)."""
    rows = 37
    x, gamma, beta = ln_inputs(rows, K, K, bf16)
    y, _ = ln_ref(x, gamma, beta, 1e-6)
    q, s = quant_rows_run(H, dev, x.to(dev), K, gamma, beta, bf16, rows, K)
    s64 = s.double()
    e_s = float(((s64 - y.abs().amax(1) / 448.0).abs() / s64).max())
    t = y / s64[:, None]
    err = (q.view(F8).double() - t).abs()
    bound = torch.maximum(2.0 ** -4 * t.abs(), torch.full_like(t, 2.0 ** -10)) + 448 * 2.0 ** -20
    print(f"quant_rows_fp8 + LayerNorm {'bf16' if bf16 else 'fp32'} K {K}: scale rel err {e_s:.2e}; |q - t| max err/bound {worst_ratio(err, bound):.3f}")
    assert e_s <= 2e-6
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements outside the bound"


@pytest.mark.parametrize("bf16", [False, True])
def test_quant_rows_fp8_layernorm_of_normalised_rows_agrees_with_plain(H, dev, bf16):
    """gamma = 1, beta = 0 on rows that are already normalised: the fused mode and the plain mode agree to one e4m3 code.  The rows
    are pairs (z, -z), scaled to a unit second moment in float64 and then stored: rounding keeps the pairs, so the mean is exactly
    zero in the kernel's fp32 sum as well (every pair cancels before the next is added), and the LayerNorm only multiplies the row by
    rstd = 1 + O(storage rounding), which the scale follows -- y / s is the same quotient up to fp32 roundings.  (Rows normalised
    without the pairing keep a mean of about 1e-4 in bf16; taking it off moves the elements near zero, where the row's codes are
    2^-9 s apart, by up to four codes -- measured -- so that input says nothing about the kernel.)  The scales agree to 2^-8 in
    bf16 (every element rounded the same way moves rstd by 2^-9) and to 2e-6 in fp32 (eps = 1e-6 alone moves rstd by 5e-7).
    Measured on the MI355X: bf16, 34 of 28 416 bytes differ, by one code, scales by 3.5e-4; fp32, no byte differs, scales by 5.4e-7."""
    rows, K = 37, 768
    torch.manual_seed(K + int(bf16))
    z = (torch.randn(rows, K // 2) * 2 + 0.5).double()
    x = torch.stack([z, -z], 2).reshape(rows, K)
    x = (x / torch.sqrt((x * x).mean(1, keepdim=True))).float()
    x = x.bfloat16() if bf16 else x
    assert bool((x[:, 0::2] == -x[:, 1::2]).all())
    xd = x.to(dev)
    q0, s0 = quant_rows_run(H, dev, xd, K, None, None, bf16, rows, K)
    q1, s1 = quant_rows_run(H, dev, xd, K, torch.ones(K), torch.zeros(K), bf16, rows, K)
    d = (e4m3_code(q0) - e4m3_code(q1)).abs()
    e_s = float(((s0 - s1).abs() / s0).max())
    print(f"quant_rows_fp8 LayerNorm vs plain on normalised {'bf16' if bf16 else 'fp32'} rows: {int((d != 0).sum())} of {d.numel()} bytes differ, "
          f"by {int(d.max())} code at most; scales differ by {e_s:.2e}")
    assert int(d.max()) <= 1
    assert e_s < (2.0 ** -8 if bf16 else 2e-6)


def test_quant_rows_fp8_refusals_leave_outputs_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    x = torch.zeros(4 * 4104 + 8, device=dev)
    g, b = torch.ones(4104, device=dev), torch.zeros(4104, device=dev)
    q = torch.full((4 * 4104,), 7, dtype=torch.uint8, device=dev)
    s = torch.full((4,), 7.0, device=dev)
    for dt in (H.F32, H.BF16):
        assert lib.cvcl_quant_rows_fp8(dt, p(x), 4104, None, None, 0.0, p(q), p(s), 4, 4104, st) == EINVAL          # K > 4096
        assert lib.cvcl_quant_rows_fp8(dt, p(x), 104, None, None, 0.0, p(q), p(s), 4, 100, st) == EINVAL            # K % 8
        assert lib.cvcl_quant_rows_fp8(dt, p(x), 768, p(g), None, 1e-6, p(q), p(s), 4, 768, st) == EINVAL           # gamma without beta
        assert lib.cvcl_quant_rows_fp8(dt, p(x), 768, None, p(b), 1e-6, p(q), p(s), 4, 768, st) == EINVAL
        assert lib.cvcl_quant_rows_fp8(dt, p(x[1:]), 768, None, None, 0.0, p(q), p(s), 4, 768, st) == EINVAL        # x off 16 bytes
    torch.cuda.synchronize()
    assert bool((q == 7).all()) and bool((s == 7.0).all())


# ---- 8. MX block quantiser ---------------------------------------------------------------------------------------------------------

def mx_input(rows, K, xs):
    """bf16 randn * 1.7 rows [rows, xs]; block 0 of rows 0 to 8 is planted: all zeros (scale byte 1 after the clamp); amax exactly
    448 (byte 127) and 448 * 2^-5 = 14 (byte 122); the next bf16 above each, 450 and 14.0625 (the exponent steps: 128, 123); a
    largest magnitude that is negative; bf16 subnormals of both signs; magnitudes near 3e38.  No infinities or NaNs."""
    torch.manual_seed(K + rows)
    x = (torch.randn(rows, xs) * 1.7).bfloat16()
    x[0, :32] = 0.0
    for r, v in ((1, 448.0), (2, 14.0), (3, 450.0), (4, 14.0625), (5, -37.5)):
        x[r, 5 + r] = v
    sub = torch.randint(1, 0x80, (32,), dtype=torch.int16)
    sub[::2] |= torch.tensor(-32768, dtype=torch.int16)
    x[6, :32] = sub.view(BF)
    x[7, :32] = (torch.randn(32) * 1e38).clamp(-3.3e38, 3.3e38).bfloat16()
    x[7, 9] = -3e38
    x[8, :32] = x[7, :32] * 2.0 ** -100                # (and an ordinary block far from 1)
    assert bool(torch.isfinite(x.float()).all())
    return x


def mx_ref(x):
    q, e, _ = _mx_quant_ref(x.float())
    return q.view(torch.uint8), _mx_tile_scales(e)


def mx_run(H, dev, xd, xs, rows, K):
    """cvcl_quant_rows_mx, the bytes three rows longer than asked for: -> (bytes [rows, K], scale bytes [K / 128, rows, 4])."""
    lib, st = H.lib(), H.stream_ptr()
    q, bs = twice(lambda: [torch.full((rows + 3, K), 0xAA, dtype=torch.uint8, device=dev),
                           torch.full((K // 128, rows, 4), 0xAA, dtype=torch.uint8, device=dev)],
                  lambda a, b: H.check(lib.cvcl_quant_rows_mx(H.ptr(xd), xs, H.ptr(a), H.ptr(b), rows, K, st), "cvcl_quant_rows_mx"))
    assert bool((q[rows:] == 0xAA).all()), "rows beyond `rows` were written"
    return q[:rows], bs


@pytest.mark.parametrize("rows,K,strided", [(37, 128, False), (1000, 128, False), (37, 768, False), (1000, 768, False),
                                            (37, 1024, False), (1000, 1024, False), (37, 768, True)])
def test_quant_rows_mx_bit_identical_to_emulation(H, dev, rows, K, strided):
    """cvcl_quant_rows_mx (quant_rows_mx_kernel, one 16-byte chunk per thread, four adjacent lanes = one block of 32): e4m3 bytes
    and e8m0 scale bytes in their [K / 128][rows][4] tiling bit-identical to _mx_quant_ref / _mx_tile_scales on the same bf16 rows.
    amax * (1 / 448) in the kernel and amax / 448 in the oracle give the same byte for every finite bf16 amax, so equality is exact.
    K = 128 is one scale tile per row, 768 and 1024 the ViT-B / ViT-L widths; the strided case reads rows at stride K + 8.  Planted
    blocks: mx_input."""
    xs = K + 8 if strided else K
    x = mx_input(rows, K, xs)
    q_ref, bs_ref = mx_ref(x[:, :K])
    assert [int(bs_ref[0, r, 0]) for r in range(5)] == [1, 127, 122, 128, 123]
    q, bs = mx_run(H, dev, x.to(dev), xs, rows, K)
    print(f"quant_rows_mx rows {rows} K {K} strided {strided}: {int((bs != bs_ref).sum())} scale bytes and {int((q != q_ref).sum())} "
          f"of {q.numel()} bytes differ")
    assert torch.equal(bs, bs_ref)
    assert torch.equal(q, q_ref)


def test_quant_rows_mx_second_grid_stride_trip(H, dev):
    """32 800 rows at K = 1024 are 4 198 400 chunks > 16384 x 256, the launch's cap: the grid-stride loop takes a second trip for the
    last 32 rows.  The input is the 1025-row case tiled 32 times, so the expected output is the small reference tiled."""
    K, small, tiles = 1024, 1025, 32
    rows = small * tiles
    assert 16384 * 256 < rows * (K // 8) < 2 * 16384 * 256
    x = mx_input(small, K, K)
    q_ref, bs_ref = mx_ref(x)
    xd = x.to(dev).repeat(tiles, 1)
    lib, st = H.lib(), H.stream_ptr()
    for _ in range(2):
        q = torch.full((rows, K), 0xAA, dtype=torch.uint8, device=dev)
        bs = torch.full((K // 128, rows, 4), 0xAA, dtype=torch.uint8, device=dev)
        H.check(lib.cvcl_quant_rows_mx(H.ptr(xd), K, H.ptr(q), H.ptr(bs), rows, K, st), "cvcl_quant_rows_mx")
        torch.cuda.synchronize()
        assert torch.equal(q, q_ref.to(dev).repeat(tiles, 1))
        assert torch.equal(bs, bs_ref.to(dev).repeat(1, tiles, 1))


def test_quant_rows_mx_refusals_leave_outputs_untouched(H, dev):
    lib, st, p = H.lib(), H.stream_ptr(), H.ptr
    x = torch.zeros(4 * 256, dtype=BF, device=dev)
    q = torch.full((4 * 256,), 7, dtype=torch.uint8, device=dev)
    bs = torch.full((2 * 4 * 4,), 7, dtype=torch.uint8, device=dev)
    assert lib.cvcl_quant_rows_mx(p(x), 64, p(q), p(bs), 4, 64, st) == EINVAL                                # K = 64
    assert lib.cvcl_quant_rows_mx(p(x), 200, p(q), p(bs), 4, 200, st) == EINVAL                              # K % 128
    assert lib.cvcl_quant_rows_mx(None, 128, p(q), p(bs), 4, 128, st) == EINVAL
    assert lib.cvcl_quant_rows_mx(p(x), 128, None, p(bs), 4, 128, st) == EINVAL
    assert lib.cvcl_quant_rows_mx(p(x), 128, p(q), None, 4, 128, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((q == 7).all()) and bool((bs == 7).all())
