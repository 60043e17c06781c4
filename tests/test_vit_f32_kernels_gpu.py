"""GPU: the fp32 ViT fine-tuning kernels (csrc/vit_f32_train.hip) against float64 on the CPU -- attention forward (O and the
log-sum-exp) and backward (dQ, dK, dV against autograd), the LayerNorm backward with the residual add, the token backward, the
fused weight / bias gradient and the GELU pieces; bit-identical reruns; refusals that leave the output untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 197, 12), (1, 257, 12), (4, 33, 2), (2, 288, 4)]
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    _hip.load()
    return _hip


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def attn_ref(qkv, d_o, heads, scale):
    """float64 autograd of vision_transformer_dino_mugs.py:106-130 on qkv [B, T, 3*heads*64]."""
    B, T, _ = qkv.shape
    x = qkv.detach().double().cpu().requires_grad_(True)
    q, k, v = x.reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-2, -1) * scale
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, heads * 64)
    o.backward(d_o.double().cpu())
    lse = torch.logsumexp(s, -1) * LOG2E
    return o.detach(), lse.detach(), x.grad


def run_attn(H, qkv, d_o, heads, scale):
    B, T, _ = qkv.shape
    lib, s = H.lib(), H.stream_ptr()
    o = torch.empty(B, T, heads * 64, device=qkv.device)
    lse = torch.empty(B, heads, T, device=qkv.device)
    H.check(lib.cvcl_attention_train_f32(H.ptr(qkv), H.ptr(o), H.ptr(lse), B, T, heads, 64, scale, s), "cvcl_attention_train_f32")
    dqkv = torch.empty_like(qkv)
    H.check(lib.cvcl_attention_bwd_f32(H.ptr(qkv), H.ptr(o), H.ptr(d_o), H.ptr(lse), H.ptr(dqkv), B, T, heads, 64, scale, s),
            "cvcl_attention_bwd_f32")
    torch.cuda.synchronize()
    return o, lse, dqkv


@pytest.mark.parametrize("B,T,heads", SHAPES)
@pytest.mark.parametrize("sharp", [False, True])
def test_attention_f32_vs_float64(H, dev, B, T, heads, sharp):
    torch.manual_seed(B * 1000 + T + heads)
    qkv = torch.randn(B, T, 3, heads, 64)
    if sharp:                       # near one-hot rows: the logits span far more than 80, the LSE path carries the softmax
        qkv[:, :, 0] *= 30.0
    qkv = qkv.reshape(B, T, -1).contiguous()
    d_o = torch.randn(B, T, heads * 64)
    scale = 64 ** -0.5
    o_r, lse_r, dq_r = attn_ref(qkv, d_o, heads, scale)
    if sharp:
        span = float((qkv.double().reshape(B, T, 3, heads, 64)[:, :, 0] @ qkv.double().reshape(B, T, 3, heads, 64)[:, :, 1].transpose(-1, -2)).abs().max()) * scale
        assert span > 80
    qkv_d, d_o_d = qkv.to(dev), d_o.to(dev)
    o, lse, dqkv = run_attn(H, qkv_d, d_o_d, heads, scale)
    # (LSE relative to its size: the logits of the sharp case reach ~1e2, and fp32 carries them to ~1e-7 relative)
    e_o, e_l = rel_l2(o, o_r), float((lse.cpu().double() - lse_r).abs().max() / (1 + lse_r.abs().max()))
    parts = [rel_l2(dqkv.reshape(B, T, 3, -1)[:, :, i], dq_r.reshape(B, T, 3, -1)[:, :, i]) for i in range(3)]
    print(f"B {B} T {T} heads {heads} sharp {sharp}: O rel-L2 {e_o:.2e}  LSE max-abs/(1+max|lse|) {e_l:.2e}  dQ/dK/dV rel-L2 "
          + " ".join(f"{p:.2e}" for p in parts))
    assert e_o < 5e-6 and e_l < 2e-6
    assert max(parts) < (2e-5 if sharp else 5e-6)
    o2, lse2, dqkv2 = run_attn(H, qkv_d, d_o_d, heads, scale)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)


def test_attention_f32_refusals_leave_outputs_untouched(H, dev):
    lib, s = H.lib(), H.stream_ptr()
    B, heads = 2, 4
    qkv = torch.randn(B, 300, 3 * heads * 64, device=dev)
    canary = torch.full((B * 300 * heads * 64 * 3,), 7.0, device=dev)
    lse = torch.full((B * heads * 300,), 7.0, device=dev)
    for hd, T in ((32, 197), (64, 32), (64, 289)):
        assert lib.cvcl_attention_train_f32(H.ptr(qkv), H.ptr(canary), H.ptr(lse), B, T, heads, hd, 0.125, s) == -1, (hd, T)
        assert lib.cvcl_attention_bwd_f32(H.ptr(qkv), H.ptr(qkv), H.ptr(qkv), H.ptr(lse), H.ptr(canary), B, T, heads, hd, 0.125, s) == -1
    assert lib.cvcl_attention_train_f32(None, H.ptr(canary), H.ptr(lse), B, 197, heads, 64, 0.125, s) == -1
    assert lib.cvcl_attention_bwd_f32(H.ptr(qkv), None, H.ptr(qkv), H.ptr(lse), H.ptr(canary), B, 197, heads, 64, 0.125, s) == -1
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all()) and bool((lse == 7.0).all())


@pytest.mark.parametrize("rows,D,stride_rows", [(1001, 768, False), (517, 128, False), (300, 1024, False), (5, 384, True)])
def test_layernorm_bwd_rows_f32_vs_float64(H, dev, rows, D, stride_rows):
    torch.manual_seed(rows + D)
    xs = D * 3 if stride_rows else D                  # strided rows: the final norm reads the cls rows of [B][T][D]
    x = torch.randn(rows, xs) * 2 + 0.5
    gamma, beta = torch.rand(D) + 0.5, torch.randn(D) * 0.1
    dy, add = torch.randn(rows, D), torch.randn(rows, xs)
    xr = x[:, :D].double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), g64, b64, 1e-6).backward(dy.double())
    lib, s = H.lib(), H.stream_ptr()
    npart = lib.cvcl_layernorm_bwd_rows_partials(rows)
    outs = []
    for _ in range(2):
        xd, dyd, addd, gd = x.to(dev), dy.to(dev), add.to(dev), gamma.to(dev)
        dx = torch.full((rows, xs), 5.0, device=dev)
        part = torch.empty(npart, 2 * D, device=dev)
        H.check(lib.cvcl_layernorm_bwd_rows_f32(H.ptr(xd), xs, H.ptr(gd), H.ptr(dyd), D, 1e-6, H.ptr(addd), H.ptr(dx), xs, H.ptr(part), rows, D,
                                                s), "cvcl_layernorm_bwd_rows_f32")
        red = torch.empty(2 * D, device=dev)
        H.check(lib.cvcl_colsum_f32(H.ptr(part), H.ptr(red), npart, 2 * D, s), "cvcl_colsum_f32")
        torch.cuda.synchronize()
        outs.append((dx.cpu(), red.cpu()))
    dx, red = outs[0]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    e_dx = rel_l2(dx[:, :D], xr.grad + add[:, :D].double())
    e_g, e_b = rel_l2(red[:D], g64.grad), rel_l2(red[D:], b64.grad)
    print(f"LN bwd rows {rows} D {D}: dx {e_dx:.2e} dgamma {e_g:.2e} dbeta {e_b:.2e}")
    assert e_dx < 2e-6 and e_g < 2e-6 and e_b < 2e-6
    if stride_rows:                                   # the columns between the rows are not written
        assert bool((dx[:, D:] == 5.0).all())


def test_vit_tokens_bwd_f32_vs_float64(H, dev):
    B, T, D = 5, 197, 192
    dh = torch.randn(B, T, D)
    lib = H.lib()
    dhd = dh.to(dev)
    d_tok = torch.empty(B * (T - 1), D, device=dev)
    d_pos = torch.empty(T, D, device=dev)
    H.check(lib.cvcl_vit_tokens_bwd_f32(H.ptr(dhd), H.ptr(d_tok), H.ptr(d_pos), B, T, D, H.stream_ptr()), "cvcl_vit_tokens_bwd_f32")
    torch.cuda.synchronize()
    assert torch.equal(d_tok.cpu(), dh[:, 1:].reshape(-1, D))
    assert rel_l2(d_pos, dh.double().sum(0)) < 1e-7


@pytest.mark.parametrize("M,N,K,k_keep", [(1000, 200, 600, 588), (3 * 197, 384, 128, 128), (16411, 96, 40, 33)])
def test_gemm_tn_colsum_f32_vs_float64(H, dev, M, N, K, k_keep):
    torch.manual_seed(M + N)
    dy, x = torch.randn(M, N), torch.randn(M, K)
    lib, s = H.lib(), H.stream_ptr()
    nb = lib.cvcl_gemm_tn_colsum_f32_workspace_bytes(M, N, K)
    runs = []
    for _ in range(2):
        dyd, xd = dy.to(dev), x.to(dev)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        dw = torch.empty(N, k_keep, device=dev)
        db = torch.empty(N, device=dev)
        H.check(lib.cvcl_gemm_tn_colsum_f32(H.ptr(dyd), N, H.ptr(xd), K, M, N, K, H.ptr(dw), k_keep, H.ptr(db), H.ptr(ws), nb, s),
                "cvcl_gemm_tn_colsum_f32")
        torch.cuda.synchronize()
        runs.append((dw.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref_w = (dy.double().t() @ x.double())[:, :k_keep]
    e_w, e_b = rel_l2(runs[0][0], ref_w), rel_l2(runs[0][1], dy.double().sum(0))
    print(f"TN M {M} N {N} K {K} k_keep {k_keep}: dW rel-L2 {e_w:.2e} db {e_b:.2e}")
    assert e_w < 2e-6 and e_b < 2e-6


def test_gelu_f32_vs_float64(H, dev):
    torch.manual_seed(3)
    u = torch.cat([torch.randn(4096) * 3, torch.linspace(-12, 12, 4096)])
    d = torch.randn_like(u)
    lib, s = H.lib(), H.stream_ptr()
    ud, dd = u.to(dev), d.to(dev)
    g, du = torch.empty_like(ud), torch.empty_like(ud)
    H.check(lib.cvcl_gelu_f32(H.ptr(ud), None, H.ptr(g), u.numel(), s), "cvcl_gelu_f32")
    H.check(lib.cvcl_gelu_f32(H.ptr(ud), H.ptr(dd), H.ptr(du), u.numel(), s), "cvcl_gelu_f32")
    torch.cuda.synchronize()
    u64 = u.double().requires_grad_(True)
    y = torch.nn.functional.gelu(u64)
    y.backward(d.double())
    # |error| / (1 + |value|): the erf form cancels in 1 + erf(u / sqrt 2) for u << 0, where fp32 (torch's CPU kernel alike) keeps
    # only the absolute accuracy of erff
    err_g = float(((g.cpu().double() - y.detach()).abs() / (1 + y.detach().abs())).max())
    err_d = float(((du.cpu().double() - u64.grad).abs() / (1 + u64.grad.abs())).max())
    print(f"GELU fp32: forward {err_g:.2e}  backward {err_d:.2e}")
    assert err_g < 1e-6 and err_d < 2e-6
