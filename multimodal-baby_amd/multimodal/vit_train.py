"""Fine-tuning path of the DINO ViT (``--finetune_cnn`` with ``--vit_dino``): the whole trunk as ONE autograd node.

Reference: vision_transformer_dino_mugs.py:87-149 (Mlp / Attention / Block) and :232-250 (prepare_tokens, forward) under
torch.autograd.  Here the forward is the frozen path's prologue (vit_hip._Trunk) and its plain block, spelled so that it keeps what
the backward needs -- the residual stream entering each norm, the normalised rows, qkv, the attention output with its log-sum-exp,
the MLP pre-activation and its GELU -- and the backward walks the blocks in reverse with explicit kernels.  Both are written once;
what differs between the two precisions, chosen by ``model.compute_dtype``, is one ``_Precision`` entry each:

bf16 (``--precision bf16``): bf16 storage, fp32 accumulation and fp32 parameter gradients.

    linear        dX = cvcl_gemm(dY, W^T copy)        dW, db = cvcl_gemm_tn_colsum(dY, X) (one pass over dY)
    attention     cvcl_attention_bwd (MFMA, probabilities rebuilt from the saved log-sum-exp)
    LayerNorm     cvcl_layernorm_bwd_rows (+ the residual gradient that bypasses the norm, in the same pass)
    GELU          in the GEMM epilogues: fc1 stores the pre-activation next to its GELU, the fc2 data-gradient GEMM multiplies
                  by gelu'(pre-activation) (cvcl_gelu_bf16 is the standalone form, kept for tests)
    tokens        cvcl_vit_tokens_bwd (patch rows -> patch-embedding weight gradient; batch sums -> pos_embed / cls_token)

fp32 (``--precision 32``, Lightning's default): fp32 storage and exact fp32 products (v_mfma_f32_32x32x2_f32) throughout.

    linear        dX = cvcl_gemm(dY, W) with the weight read K-major (w_trans)      dW, db = cvcl_gemm_tn_colsum_f32
    attention     cvcl_attention_train_f32 (forward + log-sum-exp) / cvcl_attention_bwd_f32
    LayerNorm     cvcl_layernorm_bwd_rows_f32
    GELU          a standalone pass (cvcl_gelu_f32): fc1 stores u, g = gelu(u) (the fp32 epilogue's erff expression), the
                  backward multiplies by gelu'(u) -- cvcl_gemm's bf16 epilogues stay untouched
    tokens        cvcl_vit_tokens_bwd_f32

Every kernel is deterministic.  Needs head_dim 64 and 32 < T <= 288 tokens (ViT-S/B/L at patch 16 or 14, 224 x 224) at the
native resolution.  There is no torch fallback: without the HIP library it fails."""
import collections

import torch

from . import _hip as H
from . import vit_hip

_F = torch.float32


def _transpose_bf16(w: torch.Tensor) -> torch.Tensor:
    N, K = w.shape
    out = torch.empty(K, N, dtype=w.dtype, device=w.device)
    H.check(H.lib().cvcl_transpose(H.BF16, H.ptr(w), H.ptr(out), N, K, H.stream_ptr()), "cvcl_transpose")
    return out


def _gelu_f32(u, d_y=None):
    y = torch.empty_like(u)
    H.check(H.lib().cvcl_gelu_f32(H.ptr(u), H.ptr(d_y), H.ptr(y), u.numel(), H.stream_ptr()), "cvcl_gelu_f32")
    return y


def _fc1_bf16(y2, bw):
    u = torch.empty(y2.shape[0], bw["fc1_w"].shape[0], dtype=y2.dtype, device=y2.device)
    return u, H.gemm(y2, bw["fc1_w"], bias=bw["fc1_b"], act=H.ACT_GELU, pre_out=u)      # both from the GEMM epilogue


def _fc1_f32(y2, bw):
    u = H.gemm(y2, bw["fc1_w"], bias=bw["fc1_b"])
    return u, _gelu_f32(u)


def _dgrad_bf16(dy, w, u=None):
    return H.gemm(dy, _transpose_bf16(w), gelu_grad_of=u)      # (dY W) * gelu'(u) in the epilogue


def _dgrad_f32(dy, w, u=None):
    dx = H.gemm(dy, w, w_trans=True)                            # W read K-major, no transposed copy
    return dx if u is None else _gelu_f32(u, dx)


# What differs between the precisions: the storage dtype, the library entries, ``fc1(y2, bw) -> (u, g = gelu(u))`` and
# ``dgrad(dY, W, u=None) -> dY W (* gelu'(u))``.  ``ln_bwd_dy_f32``: the entry takes dY in either dtype, named by a flag after it.
_Precision = collections.namedtuple("_Precision", "dt attention_train attention_bwd tokens_bwd wgrad ln_bwd ln_bwd_dy_f32 fc1 dgrad")
_PRECISIONS = {
    torch.bfloat16: _Precision(torch.bfloat16, "cvcl_attention_train", "cvcl_attention_bwd", "cvcl_vit_tokens_bwd", "cvcl_gemm_tn_colsum",
                               "cvcl_layernorm_bwd_rows", True, _fc1_bf16, _dgrad_bf16),
    _F: _Precision(_F, "cvcl_attention_train_f32", "cvcl_attention_bwd_f32", "cvcl_vit_tokens_bwd_f32", "cvcl_gemm_tn_colsum_f32",
                   "cvcl_layernorm_bwd_rows_f32", False, _fc1_f32, _dgrad_f32),
}


def _linear_wgrad(P, dy2d: torch.Tensor, x2d: torch.Tensor, k_keep=None):
    """-> (dW [N, k_keep], db [N]) fp32 of y = x W^T + b from one pass over dY (cvcl_gemm_tn_colsum / _f32)."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    k_keep = K if k_keep is None else k_keep
    lib = H.lib()
    nb = getattr(lib, P.wgrad + "_workspace_bytes")(M, N, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=dy2d.device)
    dw = torch.empty(N, k_keep, dtype=_F, device=dy2d.device)
    db = torch.empty(N, dtype=_F, device=dy2d.device)
    H.check(getattr(lib, P.wgrad)(H.ptr(dy2d), N, H.ptr(x2d), K, M, N, K, H.ptr(dw), k_keep, H.ptr(db), H.ptr(ws), nb, H.stream_ptr()), P.wgrad)
    return dw, db


def _ln_bwd(P, x, x_stride, gamma, dy, dy_stride, eps, add, dx, dx_stride, rows, D):
    """-> (dgamma, dbeta) fp32 [D]; dx written in place of the buffer given (+ ``add``, the gradient that bypasses the norm)."""
    lib, s = H.lib(), H.stream_ptr()
    npart = lib.cvcl_layernorm_bwd_rows_partials(rows)
    part = torch.empty(npart, 2 * D, dtype=_F, device=x.device)
    dy_f32 = (int(dy.dtype == _F),) if P.ln_bwd_dy_f32 else ()
    H.check(getattr(lib, P.ln_bwd)(H.ptr(x), x_stride, H.ptr(gamma), H.ptr(dy), *dy_f32, dy_stride, eps, H.ptr(add), H.ptr(dx), dx_stride,
                                   H.ptr(part), rows, D, s), P.ln_bwd)
    out = torch.empty(2 * D, dtype=_F, device=x.device)
    H.check(lib.cvcl_colsum_f32(H.ptr(part), H.ptr(out), npart, 2 * D, s), "cvcl_colsum_f32")
    return out[:D], out[D:]


def trunk_params(model):
    """The trunk's parameters in the order VitTrunk.backward returns their gradients (the head is applied by VisionEncoder)."""
    ps = [model.patch_embed.proj.weight, model.patch_embed.proj.bias, model.cls_token, model.pos_embed]
    for blk in model.blocks:
        ps += [blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.attn.proj.bias,
               blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias]
    ps += [model.norm.weight, model.norm.bias]
    return ps


class VitTrunk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        P = _PRECISIONS.get(model.compute_dtype)
        if P is None:
            raise NotImplementedError(f"ViT fine-tuning runs in bf16 or fp32, not {model.compute_dtype}")
        t = vit_hip._Trunk(model, x)
        if not t.native:                      # (d_pos below is the gradient of pos_embed itself, not of a resampled table)
            raise NotImplementedError("positional-embedding interpolation (non-native resolution) is not on the hot path")
        w, B, T, D, dt, cd = t.w, t.B, t.T, t.D, t.dt, t.cd
        heads = w["blocks"][0]["heads"] if w["blocks"] else 1
        if w["blocks"] and (D // heads != 64 or not 32 < T <= 288):
            raise NotImplementedError(f"ViT fine-tuning needs head_dim 64 and 32 < tokens <= 288 (got head_dim {D // heads}, {T} tokens)")
        lib, s, dev = H.lib(), H.stream_ptr(), x.device
        R = B * T
        ctx.dims = (B, T, D, T - 1, 3 * model.patch_size ** 2)
        ctx.needs = [prm is not None and prm.requires_grad for prm in params]
        h = t.tokens(work_buffers=False).h
        saved = []
        for bw in w["blocks"]:                # _Trunk.block with fresh buffers, the log-sum-exp and the MLP pre-activation u kept
            h_in = h
            y1 = torch.empty(R, D, dtype=dt, device=dev)
            vit_hip._ln(cd, h_in, D, bw["n1w"], bw["n1b"], bw["eps"], y1, False, R, D)
            qkv = H.gemm(y1, bw["qkv_w"], bias=bw["qkv_b"])
            att = torch.empty(R, D, dtype=dt, device=dev)
            lse = torch.empty(B, bw["heads"], T, dtype=_F, device=dev)
            H.check(getattr(lib, P.attention_train)(H.ptr(qkv), H.ptr(att), H.ptr(lse), B, T, bw["heads"], 64, bw["scale"], s), P.attention_train)
            h_mid = H.gemm(att, bw["proj_w"], bias=bw["proj_b"], residual=h_in)
            y2 = torch.empty(R, D, dtype=dt, device=dev)
            vit_hip._ln(cd, h_mid, D, bw["n2w"], bw["n2b"], bw["eps"], y2, False, R, D)
            u, g = P.fc1(y2, bw)
            h = H.gemm(g, bw["fc2_w"], bias=bw["fc2_b"], residual=h_mid)
            saved.append((h_in, y1, qkv, att, lse, h_mid, y2, u, g))
        cls = torch.empty(B, D, dtype=_F, device=dev)
        vit_hip._ln(cd, h, T * D, w["nw"], w["nb"], w["neps"], cls, True, B, D)
        ctx.model, ctx.w, ctx.saved, ctx.h_last, ctx.cols, ctx.precision = model, w, saved, h, t.cols, P
        return cls

    @staticmethod
    def backward(ctx, d_cls):
        w, saved, model, P = ctx.w, ctx.saved, ctx.model, ctx.precision
        B, T, D, n_p, Kpe = ctx.dims
        R = B * T
        lib, s, dev, dt = H.lib(), H.stream_ptr(), d_cls.device, P.dt
        d_cls = d_cls.contiguous().to(_F)
        # final norm on the cls rows only: dh is zero on every other token
        dh = torch.zeros(R, D, dtype=dt, device=dev)
        g_nw, g_nb = _ln_bwd(P, ctx.h_last, T * D, w["nw"], d_cls, D, w["neps"], None, dh, T * D, B, D)
        grads_blocks = []
        for bw, (h_in, y1, qkv, att, lse, h_mid, y2, u, g) in zip(reversed(w["blocks"]), reversed(saved)):
            # h_out = h_mid + fc2(gelu(fc1(norm2(h_mid))))
            d_u = P.dgrad(dh, bw["fc2_w"], u)                                   # [R, Dm]: (dh W2) * gelu'(u)
            g_fc2w, g_fc2b = _linear_wgrad(P, dh, g)
            d_y2 = P.dgrad(d_u, bw["fc1_w"])                                    # [R, D]
            g_fc1w, g_fc1b = _linear_wgrad(P, d_u, y2)
            dh_mid = torch.empty(R, D, dtype=dt, device=dev)
            g_n2w, g_n2b = _ln_bwd(P, h_mid, D, bw["n2w"], d_y2, D, bw["eps"], dh, dh_mid, D, R, D)
            # h_mid = h_in + proj(attention(qkv(norm1(h_in))))
            d_att = P.dgrad(dh_mid, bw["proj_w"])
            g_pw, g_pb = _linear_wgrad(P, dh_mid, att)
            d_qkv = torch.empty(R, 3 * D, dtype=dt, device=dev)
            H.check(getattr(lib, P.attention_bwd)(H.ptr(qkv), H.ptr(att), H.ptr(d_att), H.ptr(lse), H.ptr(d_qkv), B, T, bw["heads"], 64,
                                                  bw["scale"], s), P.attention_bwd)
            d_y1 = P.dgrad(d_qkv, bw["qkv_w"])
            g_qw, g_qb = _linear_wgrad(P, d_qkv, y1)
            if bw["qkv_b"] is None:
                g_qb = None
            dh_in = torch.empty(R, D, dtype=dt, device=dev)
            g_n1w, g_n1b = _ln_bwd(P, h_in, D, bw["n1w"], d_y1, D, bw["eps"], dh_mid, dh_in, D, R, D)
            dh = dh_in
            grads_blocks.append([g_n1w, g_n1b, g_qw, g_qb, g_pw, g_pb, g_n2w, g_n2b, g_fc1w, g_fc1b, g_fc2w, g_fc2b])
        grads_blocks.reverse()
        # tokens: h[b][0] = cls + pos[0], h[b][1 + p] = patch_embed(x)[b][p] + pos[1 + p]
        d_tok = torch.empty(B * n_p, D, dtype=dt, device=dev)
        d_pos = torch.empty(T, D, dtype=_F, device=dev)
        H.check(getattr(lib, P.tokens_bwd)(H.ptr(dh), H.ptr(d_tok), H.ptr(d_pos), B, T, D, s), P.tokens_bwd)
        g_pew, g_peb = _linear_wgrad(P, d_tok, ctx.cols, k_keep=Kpe)
        g_pew = g_pew.reshape(model.patch_embed.proj.weight.shape)
        grads = [g_pew, g_peb, d_pos[0].reshape(model.cls_token.shape).clone(), d_pos.reshape(model.pos_embed.shape)]
        for gb in grads_blocks:
            grads += gb
        grads += [g_nw, g_nb]
        grads = [g if (need and g is not None) else None for g, need in zip(grads, ctx.needs)]
        ctx.saved = ctx.h_last = ctx.cols = None
        return (None, None, *grads)


def vit_trunk_train(model, x: torch.Tensor) -> torch.Tensor:
    """Differentiable twin of vit_hip.vit_forward: cls token after the final LayerNorm, [B, D] fp32."""
    params = trunk_params(model)
    return VitTrunk.apply(model, x, *params)
