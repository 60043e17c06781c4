"""The DINO ViT's two analysis entry points on libcvcl_hip (reference multimodal/vision_transformer_dino_mugs.py:252-269):
``get_last_selfattention`` (the last block's softmax(q k^T scale), written out by csrc/vit_maps.hip) and
``get_intermediate_layers`` (the final ``norm`` of the token matrix after each of the last ``n`` blocks).

Both need the token matrix part of the way through the trunk, so this module holds a plain launch sequence of the first ``k``
blocks in the model's compute dtype (fp32 or bf16): cvcl_im2col_patches, the patch GEMM, cvcl_vit_assemble_tokens, then per block
cvcl_layernorm, the qkv GEMM, cvcl_attention, proj + residual, cvcl_layernorm, fc1 (GELU), fc2 + residual -- the kernels and the
order of the frozen forward's unfolded route (``vit_hip._vit_forward_impl``, which is not touched and stays launch for launch what
it is).  It shares ``vit_hip._packed`` (the weights cast once per weight version) and the cached resampled position table with the
forward, so non-native resolutions work as there.  It runs on the caller's stream under ``no_grad``; it does not use the
trunk-stream ring, the LayerNorm-folded GEMMs or the e4m3 linears: a model with ``fp8_linears`` takes THIS bf16 sequence, i.e. its
maps are those of the bf16 model, not of the quantised one.

In fp32 the CLS rows of ``get_intermediate_layers(x, 1)[0]`` are the bits of ``forward(x)``: the same kernels see the same rows."""
from __future__ import annotations

import torch

from . import _hip as H
from . import vit_hip


class _Trunk:
    """Token matrix h [B T, D] (compute dtype) after prepare_tokens, advanced one block at a time."""

    def __init__(self, model, x: torch.Tensor):
        if not x.is_cuda:
            raise H.CvclError("the ViT attention maps need device tensors (got a CPU tensor); there is no CPU fallback")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise H.CvclError(f"expected NCHW fp32 images, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        self.model = model
        B, _, Hh, Ww = x.shape
        p, D = model.patch_size, model.embed_dim
        self.dt = dt = model.compute_dtype
        self.cd = cd = H.cvcl_dtype(dt)
        self.lib, s = H.lib(), H.stream_ptr()
        self.gh, self.gw = Hh // p, Ww // p
        n_p = self.gh * self.gw
        self.B, self.T, self.D = B, n_p + 1, D
        T = self.T
        self.w = w = vit_hip._packed(model, dt, x.device)
        pos = w["pos"]
        if T != model.pos_embed.shape[1] or Hh != Ww:           # the forward's cache entry, same key
            key = ("pos", Hh, Ww, model.pos_embed.data_ptr(), model.pos_embed._version)
            hit = model._cache.get("pos_interp")
            if hit is None or hit[0] != key:
                probe = torch.empty(1, T, 1, device="meta")
                hit = (key, model.interpolate_pos_encoding(probe, Hh, Ww).detach().reshape(-1, D).float().contiguous())
                model._cache["pos_interp"] = hit
            pos = hit[1]
        dev = x.device
        cols = torch.empty(B * n_p, w["Kpad"], dtype=dt, device=dev)
        H.check(self.lib.cvcl_im2col_patches(cd, H.ptr(x), H.ptr(cols), B, Hh, Ww, p, w["Kpad"], s), "cvcl_im2col_patches")
        tok = H.gemm(cols, w["pe_w"], bias=w["pe_b"])
        self.h = torch.empty(B * T, D, dtype=dt, device=dev)
        H.check(self.lib.cvcl_vit_assemble_tokens(cd, H.ptr(tok), H.ptr(w["cls"]), H.ptr(pos), H.ptr(self.h), B, T, D, s),
                "cvcl_vit_assemble_tokens")
        self.y = torch.empty_like(self.h)
        self.att = torch.empty_like(self.h)
        self.qkv = torch.empty(B * T, 3 * D, dtype=dt, device=dev)
        self.mid = torch.empty(B * T, w["blocks"][0]["fc1_w"].shape[0], dtype=dt, device=dev) if w["blocks"] else None

    def qkv_of(self, bw):
        """norm1 + qkv of block ``bw`` on the current tokens -> self.qkv [B T, 3 D]."""
        vit_hip._ln(self.cd, self.h, self.D, bw["n1w"], bw["n1b"], bw["eps"], self.y, False, self.B * self.T, self.D)
        H.gemm(self.y, bw["qkv_w"], out=self.qkv, bias=bw["qkv_b"])
        return self.qkv

    def block(self, bw):
        B, T, D, h = self.B, self.T, self.D, self.h
        self.qkv_of(bw)
        H.check(self.lib.cvcl_attention(self.cd, H.ptr(self.qkv), None, H.ptr(self.att), B, T, bw["heads"], D // bw["heads"], bw["scale"],
                                        H.stream_ptr()), "cvcl_attention")
        H.gemm(self.att, bw["proj_w"], out=h, bias=bw["proj_b"], residual=h)          # h = h + proj(att)   (vit:146)
        vit_hip._ln(self.cd, h, D, bw["n2w"], bw["n2b"], bw["eps"], self.y, False, B * T, D)
        H.gemm(self.y, bw["fc1_w"], out=self.mid, bias=bw["fc1_b"], act=H.ACT_GELU)
        H.gemm(self.mid, bw["fc2_w"], out=h, bias=bw["fc2_b"], residual=h)            # h = h + mlp(...)     (vit:147)

    def normed(self):
        """The final ``norm`` of every token row, fp32 [B, T, D] (vit:268)."""
        w = self.w
        out = torch.empty(self.B, self.T, self.D, dtype=torch.float32, device=self.h.device)
        vit_hip._ln(self.cd, self.h, self.D, w["nw"], w["nb"], w["neps"], out, True, self.B * self.T, self.D)
        return out


def attention_probs(qkv: torch.Tensor, B: int, T: int, heads: int, head_dim: int, scale: float, q_rows: int | None = None) -> torch.Tensor:
    """softmax(q k^T scale) of a qkv matrix [B T, 3 heads head_dim] (fp32 or bf16) -> [B, heads, q_rows, T] fp32 for the first
    ``q_rows`` queries (default: all T)."""
    q_rows = T if q_rows is None else int(q_rows)
    if not 1 <= q_rows <= T:
        raise ValueError(f"q_rows = {q_rows} outside 1 .. T = {T}")
    if qkv.numel() != B * T * 3 * heads * head_dim:
        raise H.CvclError(f"qkv of {qkv.numel()} elements is not [B {B}][T {T}][3][heads {heads}][{head_dim}]")
    probs = torch.empty(B, heads, q_rows, T, dtype=torch.float32, device=qkv.device)
    H.check(H.lib().cvcl_attention_probs(H.cvcl_dtype(qkv.dtype), H.ptr(qkv), H.ptr(probs), B, T, heads, head_dim, float(scale), q_rows,
                                         H.stream_ptr()), "cvcl_attention_probs")
    return probs


def last_selfattention(model, x: torch.Tensor, q_rows: int | None = None):
    """-> (probs [B, heads, q_rows, T] fp32 of the LAST block, (gh, gw)): depth - 1 blocks, the last block's norm1 + qkv, then
    cvcl_attention_probs (reference :252-259)."""
    with torch.no_grad():
        t = _Trunk(model, x)
        blocks = t.w["blocks"]
        if not blocks:
            raise H.CvclError("the ViT has no blocks")
        for bw in blocks[:-1]:
            t.block(bw)
        bw = blocks[-1]
        qkv = t.qkv_of(bw)
        return attention_probs(qkv, t.B, t.T, bw["heads"], t.D // bw["heads"], bw["scale"], q_rows), (t.gh, t.gw)


def intermediate_layers(model, x: torch.Tensor, n: int = 1):
    """-> the final ``norm`` of the output of each of the last ``n`` blocks, n tensors [B, T, D] fp32 in block order (:261-269)."""
    depth = len(model.blocks)
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= depth:
        raise ValueError(f"n = {n!r} outside 1 .. depth = {depth}")
    with torch.no_grad():
        t = _Trunk(model, x)
        out = []
        for i, bw in enumerate(t.w["blocks"]):
            t.block(bw)
            if depth - i <= n:
                out.append(t.normed())
        return out


def cls_maps(probs: torch.Tensor, mean: bool) -> torch.Tensor:
    """probs [B, heads, 1, T] -> the CLS row without its CLS column: [B, T - 1] (mean over the heads) or [B, heads, T - 1]."""
    B, heads, q_rows, T = probs.shape
    if q_rows != 1:
        raise H.CvclError(f"cls_maps takes the q_rows = 1 launch, got q_rows = {q_rows}")
    out = torch.empty((B, T - 1) if mean else (B, heads, T - 1), dtype=torch.float32, device=probs.device)
    H.check(H.lib().cvcl_cls_attention_maps(H.ptr(probs, torch.float32), H.ptr(out), B, heads, T, int(bool(mean)), H.stream_ptr()),
            "cvcl_cls_attention_maps")
    return out
