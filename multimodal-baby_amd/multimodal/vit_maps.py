"""The DINO ViT's two analysis entry points on libcvcl_hip (reference multimodal/vision_transformer_dino_mugs.py:252-269):
``get_last_selfattention`` (the last block's softmax(q k^T scale), written out by csrc/vit_maps.hip) and
``get_intermediate_layers`` (the final ``norm`` of the token matrix after each of the last ``n`` blocks); and the attention
rollout over all blocks (``attention_rollout``; Abnar & Zuidema 2020, not in the reference), which shares the walk, with its
``discard_ratio`` variant (``attention_discard``, csrc/vit_discard.hip).

Both need the token matrix part of the way through the trunk, so they walk the first ``k`` blocks with ``vit_hip._Trunk``, the
frozen forward's own prologue and plain block, in the model's compute dtype (fp32 or bf16): cvcl_im2col_patches, the patch GEMM,
cvcl_vit_assemble_tokens, then per block cvcl_layernorm, the qkv GEMM, cvcl_attention, proj + residual, cvcl_layernorm, fc1 (GELU),
fc2 + residual.  With it come ``vit_hip._packed`` (the weights cast once per weight version) and the cached resampled position
table, so non-native resolutions work as in the forward.  The walk runs on the caller's stream under ``no_grad``; it does not use the
trunk-stream ring, the LayerNorm-folded GEMMs or the e4m3 linears: a model with ``fp8_linears`` takes THIS bf16 sequence, i.e. its
maps are those of the bf16 model, not of the quantised one.

The CLS rows of ``get_intermediate_layers(x, 1)[0]`` are the bits of the forward's plain route (fp32, or bf16 with ``ln_fold``
False): the same kernels see the same rows."""
from __future__ import annotations

import torch

from . import _hip as H
from .vit_hip import _Trunk


def _tokens(model, x: torch.Tensor) -> _Trunk:
    if not x.is_cuda:
        raise H.CvclError("the ViT attention maps need device tensors (got a CPU tensor); there is no CPU fallback")
    return _Trunk(model, x).tokens()


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
        t = _tokens(model, x)
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
        t = _tokens(model, x)
        out = []
        for i, bw in enumerate(t.w["blocks"]):
            t.block(bw)
            if depth - i <= n:
                out.append(t.norm())
        return out


HEAD_FUSIONS = {"mean": H.FUSE_MEAN, "max": H.FUSE_MAX, "min": H.FUSE_MIN}
ROLLOUT_SLAB_BYTES = 1 << 30         # budget of the head-fused slab [L - s, B, T, T] fp32; a larger batch is walked in chunks
ROLLOUT_MAX_T = 960                  # cvcl_attention_rollout's LDS limit


def attention_head_fuse(qkv: torch.Tensor, B: int, T: int, heads: int, head_dim: int, scale: float, head_fusion: str = "mean",
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """fuse_h softmax(q k^T scale)[b, h] of a qkv matrix [B T, 3 heads head_dim] (fp32 or bf16) -> [B, T, T] fp32
    (``head_fusion``: "mean", "max" or "min" over the heads).  The [B, heads, T, T] tensor is never written."""
    if head_fusion not in HEAD_FUSIONS:
        raise ValueError(f"head_fusion = {head_fusion!r}: one of {sorted(HEAD_FUSIONS)}")
    if qkv.numel() != B * T * 3 * heads * head_dim:
        raise H.CvclError(f"qkv of {qkv.numel()} elements is not [B {B}][T {T}][3][heads {heads}][{head_dim}]")
    if out is None:
        out = torch.empty(B, T, T, dtype=torch.float32, device=qkv.device)
    elif out.shape != (B, T, T) or not out.is_contiguous():
        raise H.CvclError(f"out {tuple(out.shape)} is not a contiguous [B {B}, T {T}, T {T}]")
    H.check(H.lib().cvcl_attention_head_fuse(H.cvcl_dtype(qkv.dtype), H.ptr(qkv), H.ptr(out, torch.float32), B, T, heads, head_dim,
                                             float(scale), HEAD_FUSIONS[head_fusion], H.stream_ptr()), "cvcl_attention_head_fuse")
    return out


def rollout_chain(fused: torch.Tensor, start_layer: int = 0, q_rows: int = 1) -> torch.Tensor:
    """fused [n, B, T, T] fp32 (block order) -> the first ``q_rows`` rows of A^_{n-1} ... A^_{start_layer}, [B, q_rows, T] fp32,
    A^_l = (F_l + I) / rowsum(F_l + I)."""
    if fused.dim() != 4 or fused.shape[2] != fused.shape[3] or fused.dtype != torch.float32 or not fused.is_contiguous():
        raise H.CvclError(f"fused {tuple(fused.shape)} {fused.dtype} is not a contiguous fp32 [n, B, T, T]")
    n, B, T, _ = fused.shape
    if not 0 <= start_layer < n:
        raise ValueError(f"start_layer = {start_layer} outside 0 .. {n - 1}")
    if not 1 <= q_rows <= T:
        raise ValueError(f"q_rows = {q_rows} outside 1 .. T = {T}")
    out = torch.empty(B, q_rows, T, dtype=torch.float32, device=fused.device)
    H.check(H.lib().cvcl_attention_rollout(H.ptr(fused, torch.float32), H.ptr(out), n, B, T, start_layer, q_rows, H.stream_ptr()),
            "cvcl_attention_rollout")
    return out


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


DISCARD_MAX_T = 4096                 # cvcl_attention_discard's limit: T T elements counted in 32 bits


def attention_discard(fused: torch.Tensor, k: int) -> torch.Tensor:
    """fused [n, B, T, T] fp32 (contiguous, non-negative), IN PLACE: in every [T, T] matrix, flattened row-major, the ``k`` smallest
    elements become +0.0 -- the first k indices of a stable ascending sort, so ties go to the lowest flat index -- except flat index
    0 (CLS -> CLS), which is never zeroed but counts towards k.  Every other element keeps its bits.  -> ``fused``.  k = 0 launches
    nothing."""
    if fused.dim() != 4 or fused.shape[2] != fused.shape[3] or fused.dtype != torch.float32 or not fused.is_contiguous():
        raise H.CvclError(f"fused {tuple(fused.shape)} {fused.dtype} is not a contiguous fp32 [n, B, T, T]")
    n, B, T, _ = fused.shape
    if not _is_int(k) or not 0 <= k <= T * T - 1:
        raise ValueError(f"k = {k!r} outside 0 .. T*T - 1 = {T * T - 1}")
    H.check(H.lib().cvcl_attention_discard(H.ptr(fused, torch.float32), n * B, T, k, H.stream_ptr()), "cvcl_attention_discard")
    return fused


def check_discard_ratio(discard_ratio) -> float:
    """``discard_ratio`` as a float: a finite int or float (no bool) with 0 <= r < 1, ValueError otherwise."""
    r = discard_ratio
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0 <= r < 1:          # (nan fails both comparisons)
        raise ValueError(f"discard_ratio = {r!r}: a number with 0 <= discard_ratio < 1")
    return float(r)


def attention_rollout(model, x: torch.Tensor, head_fusion: str = "mean", start_layer: int = 0, q_rows: int = 1,
                      slab_bytes: int | None = None, discard_ratio: float = 0.0):
    """-> (R [B, q_rows, T] fp32, (gh, gw)): the first ``q_rows`` rows of A^_L ... A^_{s+1}, s = ``start_layer``, where
    A^_l = (F_l + I) / rowsum(F_l + I) and F_l is block l's softmax(q k^T scale) fused over the heads by ``head_fusion``.  Row 0
    without column 0 is the CLS token's map over the patch grid.  One walk over the blocks: each block past ``start_layer`` has its
    qkv fused into a slab [L - s, B, T, T] (cvcl_attention_head_fuse), then one cvcl_attention_rollout launch runs the chain.  A batch
    whose slab would exceed ``slab_bytes`` (default ROLLOUT_SLAB_BYTES) is walked in chunks of images; an image's rows do not depend
    on the chunking.  The last block's attention output and MLP are not computed: nothing reads them.
    ``discard_ratio`` r > 0 (Gildenblat's vit-explain plots r = 0.9): before the chain, the k = int(T T r) weakest attentions of
    every F_l[b] are zeroed (``attention_discard``: one cvcl_attention_discard launch per slab); each block and each image is
    selected on its own.  With the default 0 nothing is launched and every output keeps its bits."""
    depth = len(model.blocks)
    ratio = check_discard_ratio(discard_ratio)
    if head_fusion not in HEAD_FUSIONS:
        raise ValueError(f"head_fusion = {head_fusion!r}: one of {sorted(HEAD_FUSIONS)}")
    if depth < 1:
        raise H.CvclError("the ViT has no blocks")
    if not _is_int(start_layer) or not 0 <= start_layer < depth:
        raise ValueError(f"start_layer = {start_layer!r} outside 0 .. depth - 1 = {depth - 1}")
    if x.dim() != 4:
        raise H.CvclError(f"expected NCHW fp32 images, got {tuple(x.shape)} {x.dtype}")
    p = model.patch_size
    B, gh, gw = x.shape[0], x.shape[2] // p, x.shape[3] // p
    T = gh * gw + 1
    if not _is_int(q_rows) or not 1 <= q_rows <= T:
        raise ValueError(f"q_rows = {q_rows!r} outside 1 .. T = {T}")
    if T > ROLLOUT_MAX_T:
        raise NotImplementedError(f"attention rollout keeps its row tile in LDS: T = {T} > {ROLLOUT_MAX_T} tokens")
    budget = ROLLOUT_SLAB_BYTES if slab_bytes is None else int(slab_bytes)
    n = depth - start_layer
    per_image = n * T * T * 4
    chunk = max(1, min(B, budget // per_image)) if B else 1
    k = int(T * T * ratio)
    with torch.no_grad():
        if not x.is_cuda:
            raise H.CvclError("the ViT attention maps need device tensors (got a CPU tensor); there is no CPU fallback")
        out = torch.empty(B, q_rows, T, dtype=torch.float32, device=x.device) if chunk < B else None
        for b0 in range(0, B, chunk):
            t = _tokens(model, x[b0:b0 + chunk])
            blocks = t.w["blocks"]
            slab = torch.empty(n, t.B, T, T, dtype=torch.float32, device=x.device)
            for i, bw in enumerate(blocks):
                fused = i >= start_layer
                if fused:
                    attention_head_fuse(t.qkv_of(bw), t.B, T, bw["heads"], t.D // bw["heads"], bw["scale"], head_fusion,
                                        out=slab[i - start_layer])
                if i + 1 < depth:
                    t.block(bw, have_qkv=fused)
            if k > 0:
                attention_discard(slab, k)
            rows = rollout_chain(slab, 0, q_rows)
            if chunk >= B:
                return rows, (gh, gw)
            out[b0:b0 + chunk] = rows
        return out, (gh, gw)


def cls_maps(probs: torch.Tensor, mean: bool) -> torch.Tensor:
    """probs [B, heads, 1, T] -> the CLS row without its CLS column: [B, T - 1] (mean over the heads) or [B, heads, T - 1]."""
    B, heads, q_rows, T = probs.shape
    if q_rows != 1:
        raise H.CvclError(f"cls_maps takes the q_rows = 1 launch, got q_rows = {q_rows}")
    out = torch.empty((B, T - 1) if mean else (B, heads, T - 1), dtype=torch.float32, device=probs.device)
    H.check(H.lib().cvcl_cls_attention_maps(H.ptr(probs, torch.float32), H.ptr(out), B, heads, T, int(bool(mean)), H.stream_ptr()),
            "cvcl_cls_attention_maps")
    return out
