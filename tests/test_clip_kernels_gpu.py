"""GPU: the kernel additions behind ``eval.py --clip_eval`` (reference eval.py:205-207, 224-226) against float64 --
the QuickGELU epilogue of cvcl_gemm / cvcl_gemm8w on each route that implements it, cvcl_attention_causal, cvcl_clip_text_pool."""
import ctypes as C

import pytest
import torch

from conftest import maxrel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    return _hip


def _quick_gelu(y):
    return y * torch.sigmoid(1.702 * y)


def _weighted(y, ref):
    """The error form of tests/test_gemm_gpu.py: |err| / (|ref| + 5 % of max |ref|), worst element."""
    err = (y.double().cpu() - ref).abs()
    return float((err / (ref.abs() + ref.abs().max() * 5e-2)).max())


# ---- QuickGELU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [False, True], ids=["bias", "bias+residual"])
def test_quick_gelu_fp32(H, dev, res):
    """fp32 cvcl_gemm (the tiled kernel's apply_act), ragged M: 3e-5 in the weighted form, the bound of test_gemm_fused_everything."""
    M, N, K = 130, 128, 64
    g = torch.Generator().manual_seed(21)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = _quick_gelu(A.double() @ W.double().t() + bias.double()) + (R.double() if res else 0)
    y = H.gemm(A.to(dev), W.to(dev), bias=bias.to(dev), act=H.ACT_QUICK_GELU, residual=R.to(dev) if res else None)
    e = _weighted(y, ref)
    print(f"[quick_gelu fp32 res={res}] weighted error {e:.3e}")
    assert y.shape == (M, N) and e < 3e-5


@pytest.mark.parametrize("res", [False, True], ids=["bias", "bias+residual"])
def test_quick_gelu_bf16_direct_to_lds(H, dev, res):
    """bf16, (256, 128, 64): the direct-to-LDS linear epilogue (K % 64 == 0, N % 128 == 0, too few tiles for the 8-wave kernel).
    Reference: float64 on the bf16 operands, rounded where the kernel stores (activation, then the residual sum).  Bound, weighted
    form: one bf16 ulp (2^-8 of the element; the kernel's fp32 value may fall on the other side of a rounding boundary) per storage
    rounding -- 8e-3 with one (test_gemm_plain's bf16 bound), 1.6e-2 with the residual's second one, where the first rounding's ulp is
    that of the possibly larger activation (test_gemm_fused_everything's bf16 bound for the same epilogue)."""
    M, N, K = 256, 128, 64
    g = torch.Generator().manual_seed(22)
    A, W = torch.randn(M, K, generator=g).bfloat16(), (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g).bfloat16()
    ref = _quick_gelu(A.double() @ W.double().t() + bias.double()).float().bfloat16().double()
    if res:
        ref = (ref + R.double()).float().bfloat16().double()
    H.prof_enable(True)
    y = H.gemm(A.to(dev), W.to(dev), bias=bias.to(dev), act=H.ACT_QUICK_GELU, residual=R.to(dev) if res else None)
    torch.cuda.synchronize()
    prof = H.prof_collect()
    H.prof_enable(False)
    assert prof.get("gemm", (0, 0))[1] == 1, prof
    e = _weighted(y, ref)
    print(f"[quick_gelu bf16 glds res={res}] weighted error {e:.3e}")
    assert y.dtype == torch.bfloat16 and e < (1.6e-2 if res else 8e-3)


def _gemm8w_args(H, A, W, Cout, bias, act, **kw):
    a = H.GemmArgs()
    M, K = A.shape
    N = W.shape[0]
    a.A, a.W, a.C = H.ptr(A), H.ptr(W), H.ptr(Cout)
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.bias, a.act = H.ptr(bias), act
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("M,N,K", [(1024, 768, 768), (3000, 3072, 768), (5000, 768, 3072), (600, 2304, 768), (50432, 768, 768), (9000, 2304, 768)])
def test_quick_gelu_gemm8w(H, dev, M, N, K):
    """cvcl_gemm8w, linear epilogue, at the shapes of test_gemm8w_linear_epilogue: float64 of the bf16 operands rounded to bf16,
    maxrel < 8e-3 (that test's bound); two runs bit-equal."""
    g = torch.Generator().manual_seed(N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    bias = torch.randn(N, generator=g)
    y = _quick_gelu(a.double() @ w.double().t() + bias.double()).float().bfloat16()
    ad, wd, bd = a.to(dev), w.to(dev), bias.to(dev)
    outs = []
    for _ in range(2):
        Cd = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        H.check(H.lib().cvcl_gemm8w(1, C.byref(_gemm8w_args(H, ad, wd, Cd, bd, H.ACT_QUICK_GELU)), H.stream_ptr()), "cvcl_gemm8w")
        outs.append(Cd)
    e = maxrel(outs[0].float(), y.float())
    print(f"[quick_gelu gemm8w {M} {N} {K}] maxrel {e:.3e}")
    assert torch.equal(outs[0], outs[1])
    assert e < 8e-3


def test_quick_gelu_through_dispatcher_takes_gemm8w(H, dev):
    """The dispatcher routes a c_fc-like block (enough 256-row tiles, K >= 256) with QuickGELU to the 8-wave kernel, and the result is
    the direct call's, bit for bit."""
    M, N, K = 256 * 24, 1024, 256
    g = torch.Generator().manual_seed(5)
    ad = torch.randn(M, K, generator=g).bfloat16().to(dev)
    wd = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().to(dev)
    bd = torch.randn(N, generator=g).to(dev)
    H.prof_enable(True)
    y = H.gemm(ad, wd, bias=bd, act=H.ACT_QUICK_GELU)
    torch.cuda.synchronize()
    prof = H.prof_collect()
    H.prof_enable(False)
    assert prof.get("gemm8w", (0, 0))[1] == 1, prof
    Cd = torch.empty_like(y)
    H.check(H.lib().cvcl_gemm8w(1, C.byref(_gemm8w_args(H, ad, wd, Cd, bd, H.ACT_QUICK_GELU)), H.stream_ptr()), "cvcl_gemm8w")
    assert torch.equal(y, Cd)


def test_quick_gelu_refused_routes_leave_output_untouched(H, dev):
    """CVCL_F32X3 and the LayerNorm-folded 8-wave form do not implement QuickGELU: non-zero return, nothing enqueued."""
    M, N, K = 65792 // 16, 1024, 256
    A32, W16 = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev).bfloat16()
    out32 = torch.full((M, N), 7.0, device=dev)
    bias = torch.zeros(N, device=dev)
    a = H.GemmArgs()
    a.A, a.W, a.C = H.ptr(A32), H.ptr(W16), H.ptr(out32)
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.act = H.ACT_QUICK_GELU
    assert H.lib().cvcl_gemm(H.F32X3, C.byref(a), H.stream_ptr()) != 0
    A16, out16 = A32.bfloat16(), torch.full((M, N), 7.0, dtype=torch.bfloat16, device=dev)
    st, cs = torch.zeros(M, 2, device=dev), torch.zeros(N, device=dev)
    b = _gemm8w_args(H, A16, W16, out16, bias, H.ACT_QUICK_GELU, ln_stats=H.ptr(st), ln_colsum=H.ptr(cs))
    assert H.lib().cvcl_gemm8w(1, C.byref(b), H.stream_ptr()) != 0
    assert H.lib().cvcl_gemm(H.BF16, C.byref(b), H.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out32 == 7.0).all()) and bool((out16 == 7.0).all())


# ---- cvcl_attention_causal --------------------------------------------------------------------------------------------------------
def _causal_ref(qkv, B, T, heads):
    q, k, v = (qkv.reshape(B, T, 3, heads, 64)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, T, heads * 64)


def _causal(H, qd, B, T, heads):
    out = torch.full((B, T, heads * 64), float("nan"), dtype=qd.dtype, device=qd.device)
    H.check(H.lib().cvcl_attention_causal(H.cvcl_dtype(qd.dtype), H.ptr(qd), H.ptr(out), B, T, heads, 64, 0.125, H.stream_ptr()),
            "cvcl_attention_causal")
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,heads", [(3, 77, 2), (2, 1, 1), (2, 5, 3)])
def test_attention_causal_vs_float64(H, dev, dtype, B, T, heads):
    """Against float64 soft-max with the upper triangle masked, on the stored (bf16: rounded) inputs.  Bounds of the generic kernel's
    existing tests: fp32 -- tau = 4 x the error of torch's own fp32 CPU evaluation (tests/vit_attention_common.py); bf16 -- 2e-2 of
    the largest output (test_attention_bf16_mfma_vs_float64, whose T = 17 case is the generic kernel)."""
    g = torch.Generator().manual_seed(T * 7 + heads)
    qkv = (torch.randn(B, T, 3 * heads * 64, generator=g) * 1.5).to(dtype)
    ref = _causal_ref(qkv.double(), B, T, heads)
    got = _causal(H, qkv.to(dev), B, T, heads).double().cpu()
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    if dtype == torch.float32:
        tau = 4.0 * float((_causal_ref(qkv, B, T, heads).double() - ref).abs().max())
        print(f"[causal f32 {B} {T} {heads}] error {err:.3e}, tau {tau:.3e}")
        assert err <= tau
    else:
        print(f"[causal bf16 {B} {T} {heads}] error / max {err / float(ref.abs().max()):.3e}")
        assert err / float(ref.abs().max()) < 2e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_attention_causal_is_causal_bit_for_bit(H, dev, dtype):
    B, T, heads, t = 2, 77, 2, 30
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, T, 3 * heads * 64, generator=g).to(dtype)
    other = qkv.clone()
    other[:, t + 1:] = (torch.randn(B, T - t - 1, 3 * heads * 64, generator=g) * 3).to(dtype)
    a, b = _causal(H, qkv.to(dev), B, T, heads), _causal(H, other.to(dev), B, T, heads)
    assert torch.equal(a[:, :t + 1], b[:, :t + 1]) and not torch.equal(a[:, t + 1:], b[:, t + 1:])


def test_attention_causal_argument_checks(H, dev):
    x = torch.zeros(16, device=dev)
    lib = H.lib()
    assert lib.cvcl_attention_causal(H.F32, H.ptr(x), H.ptr(x), 1, 8, 2, 256, 0.125, H.stream_ptr()) == -1      # head_dim > 128
    assert lib.cvcl_attention_causal(H.F32, H.ptr(x), H.ptr(x), 0, 8, 2, 64, 0.125, H.stream_ptr()) == -1
    assert lib.cvcl_attention_causal(H.F32, None, H.ptr(x), 1, 8, 2, 64, 0.125, H.stream_ptr()) == -1
    assert lib.cvcl_attention_causal(H.F32X3, H.ptr(x), H.ptr(x), 1, 8, 2, 64, 0.125, H.stream_ptr()) != 0


# ---- cvcl_clip_text_pool ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 768])
def test_clip_text_pool(H, dev, W):
    """Rows of length 2, 9 and 77 (EOT in the last slot), one row with the largest id twice (the first wins, as torch.argmax), five
    rows so that a second workgroup runs; against float64 LayerNorm of the chosen row, maxrel < 2e-6."""
    L, V = 77, 1000
    g = torch.Generator().manual_seed(W)
    tok = torch.zeros(5, L, dtype=torch.long)
    for b, n in enumerate((2, 9, 77, 40, 13)):
        tok[b, :n] = torch.randint(1, V - 1, (n,), generator=g)
        tok[b, n - 1] = V - 1
    tok[3, 17] = V - 1                                       # twice: positions 17 and 39
    want_at = torch.tensor([1, 8, 76, 17, 12])
    assert torch.equal(tok.argmax(-1), want_at)
    x = torch.randn(5, L, W, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(W, generator=g), 0.3 * torch.randn(W, generator=g)
    rows = x[torch.arange(5), want_at].double()
    ref = torch.nn.functional.layer_norm(rows, (W,), gamma.double(), beta.double(), 1e-5)
    out = torch.full((5, W), float("nan"), device=dev)
    xd, td, gd, bd = x.to(dev), tok.to(dev), gamma.to(dev), beta.to(dev)       # (named: they must outlive the launch)
    H.check(H.lib().cvcl_clip_text_pool(H.ptr(xd), H.ptr(td), H.ptr(gd), H.ptr(bd), 1e-5, H.ptr(out), 5, L, W, H.stream_ptr()),
            "cvcl_clip_text_pool")
    e = maxrel(out, ref)
    print(f"[clip_text_pool W {W}] maxrel {e:.3e}")
    assert e < 2e-6
