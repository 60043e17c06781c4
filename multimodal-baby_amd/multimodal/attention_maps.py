"""Grad-CAM attention maps and the forward-hook helper, with the reference's public names (reference
multimodal/attention_maps.py: ``Hook`` :83-105, ``gradCAM_with_act_and_grad`` :112-122, ``gradCAM`` :125-165 and the
plotting helpers :15-80).  The bodies are this repository's own.

Device work runs on libcvcl_hip (csrc/gradcam.hip): ``gradCAM`` is the reference's one forward + backward per call (the
backward reaches the hooked layer-4 map through the trunk's avgpool bridge, ``resnext._PooledFromMap``), and
``gradCAM_pairs`` is the batched form for the flat ResNeXt encoder -- one trunk pass, then every requested (image, target)
map as one exact-fp32 MFMA contraction over the layer-4 map (cvcl_hip.h, "Grad-CAM").  ``gradCAM_captions`` /
``gradCAM_for_captioning_lm`` (reference analysis_tools/multimodal_visualization.py:9-49) give one map per word of a caption for the
captioning LM: the per-word gradients of all captions come from one multi-seed BPTT sweep (csrc/lstm.hip) and feed the same
contraction.  ``overlay_attention_maps`` / ``attention_grid`` render any of these maps over their frames on the device
(csrc/overlay.hip): the batched form of ``getAttMap``.  The reference's own plotting helpers (``getAttMap``, ``preprocess_attn_map``,
``plot_image``) stay host-side
numpy / matplotlib; matplotlib and scipy are imported only when a helper needs them."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _hip as H
from . import ops
from .multimodal_data_module import PAD_TOKEN_ID

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class Hook:
    """Captures what ``module`` returns on its next forward call(s); with ``requires_grad`` the captured tensor is made a
    gradient-retaining leaf of the graph that follows, so ``gradient`` is available after a backward pass.  Leaving the
    ``with`` block detaches the hook from the module."""

    def __init__(self, module: nn.Module, requires_grad: bool = True):
        self.requires_grad = bool(requires_grad)
        self.data: Optional[torch.Tensor] = None

        def capture(_module, _inputs, output):
            if self.requires_grad:
                output.requires_grad_(True).retain_grad()
            self.data = output

        self.hook = module.register_forward_hook(capture)

    def __enter__(self) -> "Hook":
        return self

    def __exit__(self, *exc) -> None:
        self.hook.remove()

    activation = property(lambda self: self.data, doc="the captured output tensor (None before the first forward)")
    gradient = property(lambda self: self.data.grad, doc="d loss / d activation after backward (requires_grad=True)")


# ---- device side ---------------------------------------------------------------------------------------------------------

def _nhwc_flag(t: torch.Tensor) -> int:
    """0: NCHW-contiguous, 1: channels-last storage (the trunk's layer-4 view); anything else is refused."""
    if t.dim() != 4:
        raise H.CvclError(f"expected an [N, C, h, w] tensor, got {tuple(t.shape)}")
    if t.is_contiguous():
        return 0
    if t.permute(0, 2, 3, 1).is_contiguous():
        return 1
    raise H.CvclError("act / grad must be NCHW-contiguous or channels-last")


def gradCAM_with_act_and_grad(act: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    """relu(sum_c mean_hw(grad)[c] act[c]) -> [N, 1, h, w] fp32 (reference :112-122) for any layer's act / grad, fp32 or bf16,
    NCHW or channels-last."""
    if not (act.is_cuda and grad.is_cuda):
        raise H.CvclError("gradCAM_with_act_and_grad needs device tensors (there is no CPU fallback)")
    if act.shape != grad.shape:
        raise H.CvclError(f"act {tuple(act.shape)} and grad {tuple(grad.shape)} differ in shape")
    N, C, h, w = act.shape
    fa, fg = _nhwc_flag(act), _nhwc_flag(grad)
    cam = torch.empty(N, 1, h, w, dtype=torch.float32, device=act.device)
    p_act, p_grad = (H.ptr(t.permute(0, 2, 3, 1) if nhwc else t) for t, nhwc in ((act, fa), (grad, fg)))
    H.check(H.lib().cvcl_gradcam_act_grad(H.cvcl_dtype(act.dtype), p_act, fa, H.cvcl_dtype(grad.dtype), p_grad, fg,
                                          H.ptr(cam), N, C, h * w, H.stream_ptr()), "cvcl_gradcam_act_grad")
    return cam


def bicubic_resize(x: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(x, size, mode='bicubic', align_corners=False) over the last two dimensions of an fp32 tensor."""
    Hh, Ww = int(size[0]), int(size[1])
    x = x.contiguous()
    h, w = x.shape[-2:]
    maps = x.numel() // (h * w)
    y = torch.empty(*x.shape[:-2], Hh, Ww, dtype=torch.float32, device=x.device)
    H.check(H.lib().cvcl_bicubic_resize(H.ptr(x, torch.float32), H.ptr(y), maps, h, w, Hh, Ww, H.stream_ptr()), "cvcl_bicubic_resize")
    return y


def gradCAM(model: nn.Module, input: torch.Tensor, target: torch.Tensor, layer: nn.Module, normalize_features: bool = False,
            resize: bool = True) -> torch.Tensor:
    """Reference :125-165: one forward + backward of ``model`` (the vision encoder's ResNeXt) with ``layer`` hooked; returns
    [N, 1, H, W] fp32 (``resize``: bicubic to the input's size) or [N, 1, h, w].  A batch of N images with N targets gives the
    row-wise (diagonal) pairs.  Every parameter's ``requires_grad`` is switched off for the call and restored afterwards."""
    if input.grad is not None:
        input.grad.zero_()
    saved = {name: p.requires_grad for name, p in model.named_parameters()}
    for p in model.parameters():
        p.requires_grad_(False)
    if not isinstance(layer, nn.Module):
        raise TypeError("layer must be an nn.Module")
    try:
        with Hook(layer) as hook, torch.enable_grad():
            output = model(input)
            if normalize_features:
                output = ops.l2_normalize(output)
            output.backward(target)
            act, grad = hook.activation, hook.gradient
    finally:
        for name, p in model.named_parameters():
            p.requires_grad_(saved[name])
    if grad is None:
        raise H.CvclError("no gradient reached the hooked layer")
    cam = gradCAM_with_act_and_grad(act.detach(), grad)
    if resize:
        cam = bicubic_resize(cam, input.shape[2:])
    return cam


def _resnet_of(vision_model):
    """The flat ResNeXt behind ``vision_model`` (a VisionEncoder or its ``.model``); NotImplementedError for the encoders the
    reference's gradCAM cannot run on either."""
    from .resnext import ResNet, SpatialResNet
    if getattr(vision_model, "vit_dino", False):
        raise NotImplementedError("Grad-CAM is defined for the ResNeXt encoder only (the ViT encoder has no layer4 map)")
    if getattr(vision_model, "embedding_type", None) == "spatial":
        raise NotImplementedError("Grad-CAM is not defined for embedding_type spatial (no pooled fc output to differentiate)")
    model = getattr(vision_model, "model", vision_model)
    if isinstance(model, SpatialResNet):
        raise NotImplementedError("Grad-CAM is not defined for embedding_type spatial (no pooled fc output to differentiate)")
    if not isinstance(model, ResNet) or not isinstance(model.fc, nn.Linear):
        raise NotImplementedError(f"Grad-CAM is defined for the ResNeXt encoder with a linear fc only (got {type(model).__name__})")
    return model


def _parse_pairs(pairs, N, M):
    """-> (mode, k, output shape prefix)."""
    if pairs == "all":
        return H.GRADCAM_ALL, 0, (N, M)
    if pairs == "diagonal":
        if M != N:
            raise ValueError(f"diagonal pairs need as many targets as images (N {N}, M {M})")
        return H.GRADCAM_BLOCK_IMAGE, 1, (N,)
    if isinstance(pairs, (tuple, list)) and len(pairs) == 3 and pairs[0] == "block" and pairs[2] in ("image", "text"):
        k = int(pairs[1])
        if pairs[2] == "image":
            if k <= 0 or M != N * k:
                raise ValueError(f"('block', {k}, 'image') pairs image n with targets n k .. n k + k - 1: needs M = N k (N {N}, M {M})")
            return H.GRADCAM_BLOCK_IMAGE, k, (N, k)
        if k <= 0 or N != M * k:
            raise ValueError(f"('block', {k}, 'text') pairs target j with images j k .. j k + k - 1: needs N = M k (N {N}, M {M})")
        return H.GRADCAM_BLOCK_TEXT, k, (M, k)
    raise ValueError(f"pairs must be 'all', 'diagonal' or ('block', k, 'image' | 'text'), got {pairs!r}")


def gradcam_from_features(fmap, features, fc_weight, targets, normalize_features=False, pairs="all", resize=False, eps=1e-12):
    """Grad-CAM maps from one trunk pass's outputs: ``fmap`` the layer-4 map ([N, C, h, w] view of NHWC storage), ``features``
    [N, E] = fc(pooled) of the same pass, ``fc_weight`` [E, C], ``targets`` [M, E].  See gradCAM_pairs for pairs / resize."""
    for t in (fmap, features, fc_weight, targets):
        if not t.is_cuda:
            raise H.CvclError("Grad-CAM needs device tensors (got a CPU tensor); there is no CPU fallback")
    N, C, h, w = fmap.shape
    rows = fmap.permute(0, 2, 3, 1)
    if not rows.is_contiguous():
        raise H.CvclError("the layer-4 map must be channels-last storage (the trunk's output)")
    f = features.detach().contiguous()
    W = fc_weight.detach().contiguous()
    T = targets.detach().to(torch.float32).contiguous()
    M = T.shape[0]
    if f.shape != (N, W.shape[0]) or T.shape[1] != W.shape[0] or W.shape[1] != C:
        raise H.CvclError(f"shapes: map {tuple(fmap.shape)}, features {tuple(f.shape)}, fc weight {tuple(W.shape)}, targets {tuple(T.shape)}")
    mode, k, prefix = _parse_pairs(pairs, N, M)
    P = H.gemm(T, W, w_trans=True)                             # [M, C] = T W
    Q = S = norm = None
    if normalize_features:
        y = torch.empty_like(f)
        norm = torch.empty(N, dtype=torch.float32, device=f.device)
        H.check(H.lib().cvcl_l2norm_fwd(H.ptr(f, torch.float32), H.ptr(y), H.ptr(norm), N, f.shape[1], eps, H.stream_ptr()), "cvcl_l2norm_fwd")
        S = H.gemm(y, T)                                       # [N, M] = n^ . t
        Q = H.gemm(y, W, w_trans=True)                         # [N, C] = n^ W
    cam = torch.empty(*prefix, h, w, dtype=torch.float32, device=f.device)
    H.check(H.lib().cvcl_gradcam_pairs(H.cvcl_dtype(fmap.dtype), H.ptr(rows), N, h * w, C, H.ptr(P), M, mode, k, H.ptr(Q), H.ptr(S),
                                       H.ptr(norm), eps, H.ptr(cam), H.stream_ptr()), "cvcl_gradcam_pairs")
    if resize is not False and resize is not None:
        if resize is True:
            raise ValueError("resize=True needs the input images' size: pass resize=(H, W)")
        cam = bicubic_resize(cam, resize)
    return cam


@torch.no_grad()
def gradCAM_pairs(vision_model, images, targets, normalize_features=False, pairs="all", resize=False):
    """Batched Grad-CAM of the flat ResNeXt encoder: one trunk pass over ``images`` [N, 3, H, W], then the maps of the requested
    (image, target) pairs for ``targets`` [M, E] -- the values gradCAM(model, image, target, model.layer4, normalize_features)
    gives pair by pair, without a backward pass.
      pairs = "all"                    -> [N, M, h, w]
              "diagonal" (M = N)       -> [N, h, w]      image n with target n
              ("block", k, "image")    -> [N, k, h, w]   image n with targets n k .. n k + k - 1  (M = N k)
              ("block", k, "text")     -> [M, k, h, w]   target j with images j k .. j k + k - 1  (N = M k)
      resize = False | True (bicubic to H x W) | (H', W')."""
    resnet = _resnet_of(vision_model)
    if not (images.is_cuda and targets.is_cuda):
        raise H.CvclError("gradCAM_pairs needs device tensors (got a CPU tensor); there is no CPU fallback")
    with Hook(resnet.layer4, requires_grad=False) as hook:
        features = resnet(images)
        fmap = hook.activation
    size = tuple(images.shape[2:]) if resize is True else resize
    return gradcam_from_features(fmap, features, resnet.fc.weight, targets, normalize_features, pairs, size)


# ---- self-attention maps of the DINO ViT encoder ---------------------------------------------------------------------------

def _vit_of(vision_model):
    """The VisionTransformer behind ``vision_model`` (a VisionEncoder or the ViT itself); a ResNeXt encoder is sent to Grad-CAM."""
    from .vision_transformer_dino_mugs import VisionTransformer
    model = getattr(vision_model, "model", vision_model)
    if not isinstance(model, VisionTransformer):
        raise NotImplementedError("self-attention maps are defined for the ViT encoder only; for the ResNeXt encoder use gradCAM_pairs "
                                  f"(got {type(model).__name__})")
    return model


@torch.no_grad()
def vit_cls_attention(vision_model, x, size=None, heads="mean"):
    """The CLS query's attention over the patch tokens in the ViT's last block (the usual view of a DINO ViT; the CLS row of
    reference vision_transformer_dino_mugs.py:252-259 without its CLS column): [B, gh, gw] fp32 averaged over the heads
    (``heads="mean"``) or [B, heads, gh, gw] (``heads=None``).  One q_rows = 1 launch of cvcl_attention_probs: the T x T matrix is
    never formed.  ``size=(H, W)``: resized bicubically (cvcl_bicubic_resize).  Unlike Grad-CAM the map does not depend on a target."""
    from . import vit_maps
    vit = _vit_of(vision_model)
    if heads not in ("mean", None):
        raise ValueError(f"heads = {heads!r}: 'mean' or None")
    if not x.is_cuda:
        raise H.CvclError("vit_cls_attention needs device tensors (got a CPU tensor); there is no CPU fallback")
    probs, (gh, gw) = vit_maps.last_selfattention(vit, x, q_rows=1)
    maps = vit_maps.cls_maps(probs, heads == "mean")
    maps = maps.view(*maps.shape[:-1], gh, gw)
    if size is not None:
        maps = bicubic_resize(maps, size)
    return maps


@torch.no_grad()
def vit_attention_rollout(vision_model, x, size=None, head_fusion="mean", start_layer=0):
    """The CLS token's attention rollout over the patch tokens (Abnar & Zuidema 2020): row 0, without column 0, of
    A^_L ... A^_{start_layer + 1} with A^_l = (F_l + I) / rowsum(F_l + I), F_l block l's attention fused over the heads
    (``head_fusion``: "mean", "max", "min") -> [B, gh, gw] fp32.  Where vit_cls_attention shows the last block's mixing step alone,
    this attributes the CLS token to the input patches through every block and the residual paths.  Each map sums to 1 - R[0, 0].
    ``size=(H, W)``: resized bicubically (cvcl_bicubic_resize).  The ``discard_ratio`` variant (the weakest attentions of every
    block zeroed before the chain) is vit_attention_rollout_discard below."""
    return vit_attention_rollout_discard(vision_model, x, 0.0, size, head_fusion, start_layer)


@torch.no_grad()
def vit_attention_rollout_discard(vision_model, x, discard_ratio, size=None, head_fusion="mean", start_layer=0):
    """vit_attention_rollout in the form people plot (Gildenblat's vit-explain, ``discard_ratio`` 0.9): in every block's fused
    attention F_l[b], flattened to T T elements, the k = int(T T discard_ratio) smallest are set to zero before (F_l + I) is
    normalised and chained -- ties go to the lowest flat index; element 0 (CLS -> CLS) is kept but counts towards k; each block and
    each image is selected on its own (the original masks batch element 0 only: a bug not copied).  Without it the rollout of a
    12-block ViT is close to uniform.  0 <= discard_ratio < 1, ValueError otherwise; 0 is vit_attention_rollout bit for bit.
    -> [B, gh, gw] fp32; each map still sums to 1 - R[0, 0]."""
    from . import vit_maps
    vit_maps.check_discard_ratio(discard_ratio)
    vit = _vit_of(vision_model)
    rows, (gh, gw) = vit_maps.attention_rollout(vit, x, head_fusion, start_layer, q_rows=1, discard_ratio=discard_ratio)
    maps = rows[:, 0, 1:].contiguous().view(-1, gh, gw)
    if size is not None:
        maps = bicubic_resize(maps, size)
    return maps


# ---- per-word maps of the captioning language model ----------------------------------------------------------------------

# caption_seed_targets' own bound on the caption length: the one text_train.transformer_text_train puts on utterances.  The LSTM
# functions it runs on (ops.lstm_recurrence, cvcl_lstm_cell_bwd_seeds) take any length.
MAX_CAPTION_LEN = 32


def _captioning_lstm_of(language_model):
    """The text encoder behind ``language_model`` when it is the captioning one-layer uni-directional LSTM; refusals otherwise."""
    te = getattr(language_model, "text_encoder", None)
    if te is None or not hasattr(language_model, "output_layer"):
        raise TypeError("expected a LanguageModel (text_encoder + output_layer)")
    if getattr(te, "has_attention", False):
        raise NotImplementedError("attention language models are outside the implemented path")
    if not getattr(te, "captioning", False):
        raise NotImplementedError("per-word Grad-CAM needs a captioning text encoder (--captioning: the LSTM starts from the image)")
    lstm = getattr(te, "lstm", None)
    if te.text_encoder != "lstm" or lstm is None or lstm.num_layers != 1 or lstm.bidirectional:
        raise NotImplementedError("per-word Grad-CAM is defined for the one-layer uni-directional LSTM text encoder only")
    return te


def caption_seed_targets(features, language_model, y, y_len, normalize_features=False, eps=1e-12):
    """-> targets [B (L-1), E] fp32, row b (L-1) + p = -d loss[b, p] / d f[b]: minus the gradient of the token-wise captioning loss
    (``LanguageModel.calculate_ce_loss(y, y_len, image_features=n, tokenwise=True)``, n = f or F.normalize(f)) wrt the fc output
    ``features`` [B, E], for every caption and position at once and without an autograd graph.  Zero rows where the label is <pad>.

    One LSTM forward that saves gate activations and cell states, unit seeds through the output layer (the seeds are -1, so every
    later quantity is already the negated one), then L - 1 steps of a triangular sweep -- one cvcl_lstm_cell_bwd_seeds launch and
    one recurrent GEMM over all chains alive at that step -- and the connector / normalisation backward on all rows.  Always the
    eval arithmetic: no dropout_i mask is drawn, whatever the modules' ``training`` flags say."""
    te = _captioning_lstm_of(language_model)
    if y.dim() != 2 or y_len.shape != (y.shape[0],) or features.shape[0] != y.shape[0]:
        raise H.CvclError(f"shapes: features {tuple(features.shape)}, y {tuple(y.shape)}, y_len {tuple(y_len.shape)}")
    B, L = y.shape
    if L > MAX_CAPTION_LEN:
        raise NotImplementedError(f"captions are at most {MAX_CAPTION_LEN} tokens on the LSTM path; got L = {L}")
    if L < 2:
        raise ValueError("a caption needs at least two tokens: position p predicts token p + 1")
    for t in (features, y, y_len):
        if not t.is_cuda:
            raise H.CvclError("per-word Grad-CAM needs device tensors (got a CPU tensor); there is no CPU fallback")
    F32 = torch.float32
    lib, s, dev = H.lib(), H.stream_ptr(), features.device
    lstm, Hd, K = te.lstm, te.hidden_dim, L - 1
    table = te.embedding.weight.detach().contiguous()
    V, E = table.shape
    if Hd % 4 != 0:
        raise H.CvclError(f"hidden_dim {Hd} is not a multiple of 4")
    y = y.to(torch.int64).contiguous()
    length = y_len.to(torch.int64).contiguous()
    f = features.detach().to(F32).contiguous()
    n, norm = f, None
    if normalize_features:                                                          # encode_image (reference multimodal.py:736)
        n = torch.empty_like(f)
        norm = torch.empty(B, dtype=F32, device=dev)
        H.check(lib.cvcl_l2norm_fwd(H.ptr(f), H.ptr(n), H.ptr(norm), B, E, eps, s), "cvcl_l2norm_fwd")

    # forward: connector -> (h0, c0), the LSTM over tokens 0 .. L-2 with everything BPTT needs saved, output layer, softmax
    w_conn = te.connector.weight.detach().contiguous()                              # [2 H, E]
    state = H.gemm(n, w_conn, bias=te.connector.bias.detach().contiguous())
    c0 = state[:, Hd:].contiguous()
    x = ops._embed_gather(table, y[:, :K].contiguous())
    w_hh = lstm.weight_hh_l0.detach().contiguous()
    gx = H.gemm(x, lstm.weight_ih_l0.detach().contiguous(), bias=(lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().contiguous())
    hc = ops.lstm_initial_state(state[:, :Hd], c0, B, Hd, dev)
    out, gact, csave, _ = ops.lstm_recurrence(gx, w_hh, length, hc, B, K, save=True)
    w_out = language_model.output_layer.weight.detach().contiguous()                # [V, H] (the tied table)
    b_out = language_model.output_layer.bias
    logits = H.gemm(out, w_out, bias=None if b_out is None else b_out.detach().contiguous())
    labels = y[:, 1:].contiguous().view(-1)
    R = B * K
    loss = torch.empty(R, dtype=F32, device=dev)
    lse = torch.empty(R, dtype=F32, device=dev)
    H.check(lib.cvcl_token_ce_fwd(H.ptr(logits), H.ptr(labels), H.ptr(loss), H.ptr(lse), R, V, PAD_TOKEN_ID, s), "cvcl_token_ce_fwd")

    # seeds: -(softmax - onehot) per token (unit upstream gradient, negated), through the output layer
    minus_one = torch.full((R,), -1.0, dtype=F32, device=dev)
    d_logits = torch.empty_like(logits)
    H.check(lib.cvcl_token_ce_bwd(H.ptr(logits), H.ptr(labels), H.ptr(lse), H.ptr(minus_one), H.ptr(d_logits), R, V, PAD_TOKEN_ID, s),
            "cvcl_token_ce_bwd")
    d_out = H.gemm(d_logits, w_out, w_trans=True)                                   # [B K, H], row b K + p

    # triangular sweep over the seed-major state [K][B][H]: at step t the chains of blocks t .. K-1 are alive
    dh = torch.empty(K * B, Hd, dtype=F32, device=dev)
    dc = torch.empty(K * B, Hd, dtype=F32, device=dev)
    dG = torch.empty(K * B, 4 * Hd, dtype=F32, device=dev)
    carry = torch.empty(K * B, Hd, dtype=F32, device=dev)
    for t in range(K - 1, -1, -1):
        rows, alive_h, alive_c = B * (K - t), dh[t * B:], dc[t * B:]
        H.check(lib.cvcl_lstm_cell_bwd_seeds(H.ptr(gact), H.ptr(csave), H.ptr(c0) if t == 0 else None, H.ptr(length), t, H.ptr(d_out),
                                             H.ptr(alive_h), H.ptr(alive_c), H.ptr(dG), H.ptr(carry), B, K, Hd, rows, s),
                "cvcl_lstm_cell_bwd_seeds")
        H.gemm(dG, w_hh, M=rows, w_trans=True, residual=carry, out=alive_h, stream=s)   # dh_{t-1} = dG_t . W_hh + carry

    # connector backward on all rows: d n = dh0 W[:H] + dc0 W[H:], then F.normalize's backward with the image's (n, norm) and the
    # reordering seed-major -> image-major in one launch
    dn = H.gemm(dc, w_conn[Hd:], w_trans=True, residual=H.gemm(dh, w_conn[:Hd], w_trans=True))
    targets = torch.empty(B * K, E, dtype=F32, device=dev)
    H.check(lib.cvcl_l2norm_bwd_seeds(H.ptr(n) if normalize_features else None, H.ptr(norm), H.ptr(dn), H.ptr(targets), B, K, E, eps, s),
            "cvcl_l2norm_bwd_seeds")
    return targets


def caption_gradcam_from_features(fmap, features, fc_weight, language_model, y, y_len, normalize_features=False, resize=False):
    """Per-word Grad-CAM maps of a captioning LM from one trunk pass's outputs -> [B, L-1, h, w] fp32 (or [B, L-1, H', W'] with
    ``resize=(H', W')``): map [b, p] is relu(sum_c alpha_c A[b, c]) with alpha = -mean_hw d loss[b, p] / d A[b], loss[b, p] the cross
    entropy of predicting y[b, p + 1] from position p -- what the reference's gradCAM_for_captioning_lm returns for step p + 1
    (analysis_tools/multimodal_visualization.py:9-49), for all captions and words without a backward pass per word.  ``fmap``,
    ``features``, ``fc_weight`` as in gradcam_from_features; ``y`` [B, L] int64, ``y_len`` [B].  Maps of <pad> labels are exactly 0.
    The map reaches the loss only through avgpool and fc, so the maps are the Grad-CAM contraction (cvcl_gradcam_pairs, image n with
    its own L - 1 targets) of the targets caption_seed_targets computes; the normalisation is already inside them."""
    for t in (fmap, features, fc_weight):
        if not t.is_cuda:
            raise H.CvclError("per-word Grad-CAM needs device tensors (got a CPU tensor); there is no CPU fallback")
    targets = caption_seed_targets(features, language_model, y, y_len, normalize_features)
    return gradcam_from_features(fmap, features, fc_weight, targets, False, ("block", y.shape[1] - 1, "image"), resize)


@torch.no_grad()
def gradCAM_captions(model, images, y, y_len, resize=False):
    """Batched per-word Grad-CAM of a captioning ``MultiModalLitModel``: one eval-mode trunk pass over ``images`` [B, 3, H, W], then
    caption_gradcam_from_features with the model's ``normalize_features`` -> [B, L-1, h, w] (``resize=True``: bicubic to H x W).
    Flat ResNeXt encoder + captioning one-layer LSTM only.  No autograd graph is built; every ``requires_grad``, ``training`` flag and
    parameter ``.grad`` is left as it was found (the trunk runs with its modules in eval mode for the length of the pass, as the
    reference calls this on an eval() model; the language model's arithmetic is the eval one whatever its flags)."""
    resnet = _resnet_of(model.vision_encoder)
    _captioning_lstm_of(model.language_model)
    for t in (images, y, y_len):
        if not t.is_cuda:
            raise H.CvclError("gradCAM_captions needs device tensors (got a CPU tensor); there is no CPU fallback")
    flags = [(m, m.training) for m in resnet.modules()]
    try:
        for m, _ in flags:
            m.training = False
        with Hook(resnet.layer4, requires_grad=False) as hook:
            features = resnet(images)
            fmap = hook.activation
    finally:
        for m, was in flags:
            m.training = was
    size = tuple(images.shape[2:]) if resize is True else resize
    return caption_gradcam_from_features(fmap, features, resnet.fc.weight, model.language_model, y, y_len,
                                         bool(model.model.normalize_features), size)


def gradCAM_for_captioning_lm(model, x, y, y_len, steps=None):
    """The reference's call (analysis_tools/multimodal_visualization.py:9-49): one image ``x`` [3, H, W], one caption ``y`` [L] with
    ``y_len`` (a one-element tensor) -> a list over ``steps`` (default 0 .. y_len - 1): None for step 0, otherwise the [h, w] numpy
    map of predicting word ``step``.  A batch-of-one call of gradCAM_captions."""
    if steps is None:
        steps = list(range(int(y_len.item())))
    dev = next(model.parameters()).device
    cams = gradCAM_captions(model, x.unsqueeze(0).to(dev), y.unsqueeze(0).to(dev), y_len.reshape(1).to(dev))[0]
    host = cams.cpu().numpy()
    return [None if step == 0 else host[step - 1] for step in steps]


# ---- overlays on the device (csrc/overlay.hip) ---------------------------------------------------------------------------

_LUT_CACHE = {}                                             # (colormap name, device) -> [n, 3] fp32 device tensor


def resolve_lut(cmap) -> np.ndarray:
    """The [n, 3] float32 colour table of ``cmap``: a matplotlib colormap name (``cm(np.arange(cm.N))[:, :3]``; matplotlib is imported
    here, only for a name that colormaps.BUILTIN does not hold -- "viridis", the default, is built in with matplotlib's own values) or
    an explicit [n, 3] array / tensor of RGB values, 2 <= n <= 1024."""
    from .colormaps import BUILTIN
    if isinstance(cmap, str) and cmap in BUILTIN:
        lut = np.asarray(BUILTIN[cmap], dtype=np.float64)
    elif isinstance(cmap, str):
        try:
            import matplotlib
        except ImportError as e:
            raise H.CvclError(f"cmap {cmap!r} is a matplotlib name and matplotlib is missing ({e}); pass an [n, 3] array instead") from e
        cm = matplotlib.colormaps[cmap]
        lut = cm(np.arange(cm.N))[:, :3]
    else:
        lut = cmap.detach().cpu().numpy() if torch.is_tensor(cmap) else np.asarray(cmap)
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    if lut.ndim != 2 or lut.shape[1] != 3 or not 2 <= lut.shape[0] <= 1024:
        raise ValueError(f"a colour table is [n, 3] with 2 <= n <= 1024, got {lut.shape}")
    return lut


def device_lut(cmap, device) -> torch.Tensor:
    """resolve_lut on ``device``; a colormap NAME is resolved and uploaded once per (name, device)."""
    device = torch.device(device)
    if not isinstance(cmap, str):
        return torch.from_numpy(resolve_lut(cmap)).to(device)
    index = torch.cuda.current_device() if device.type == "cuda" and device.index is None else device.index
    key = (cmap, device.type, index)
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.from_numpy(resolve_lut(cmap)).to(device)
    return _LUT_CACHE[key]


def grid_geometry(n_tiles: int, H: int, W: int, nrow: int = 4, padding: int = 2):
    """torchvision.utils.make_grid's layout of ``n_tiles`` >= 2 tiles of H x W: -> (Hc, Wc, [(y, x) of every tile's top-left pixel]).
    min(nrow, n_tiles) tiles per row, ``padding`` pixels between tiles and around the canvas, a ragged last row left empty."""
    if n_tiles < 1 or nrow < 1 or padding < 0 or H < 1 or W < 1:
        raise ValueError(f"grid of {n_tiles} tiles of {H} x {W}, nrow {nrow}, padding {padding}")
    xmaps = min(nrow, n_tiles)
    ymaps = -(-n_tiles // xmaps)
    th, tw = H + padding, W + padding
    return th * ymaps + padding, tw * xmaps + padding, [((k // xmaps) * th + padding, (k % xmaps) * tw + padding) for k in range(n_tiles)]


def _overlay_launch(images, maps, image_of_map, lut, flags, gamma, vmin, vmax, mean, std, dst_offset, pitch, out_f32, out_u8, out_map):
    """One cvcl_attn_overlay call; ``maps`` [M, h, w] (None with OVERLAY_IMAGE_ONLY: one tile per entry of the destination table)."""
    import ctypes
    N, _, Hh, Ww = images.shape
    if maps is None:
        M, h, w = (dst_offset.numel() if dst_offset is not None else N), Hh, Ww
    else:
        M, h, w = maps.shape
    lib = H.lib()
    need = lib.cvcl_attn_overlay_workspace_bytes(M, h, w, Hh, Ww, flags)
    if need == 0:
        raise H.CvclError(f"attention overlays: {M} maps of {h} x {w} on frames of {Hh} x {Ww} are outside the limits "
                          "(1 <= H, W <= 1024, 1 <= h <= H, 1 <= w <= W)")
    ws = torch.empty(need, dtype=torch.uint8, device=images.device)
    colour = out_f32 if out_f32 is not None else out_u8
    mean_c, std_c = ((ctypes.c_float * 3)(*(float(v) for v in t)) for t in (mean, std))     # host arrays, read during the call
    H.check(lib.cvcl_attn_overlay(H.ptr(maps, torch.float32), M, h, w, H.ptr(images, torch.float32), N, Hh, Ww, ctypes.cast(mean_c, ctypes.c_void_p),
                                  ctypes.cast(std_c, ctypes.c_void_p),
                                  H.ptr(image_of_map, torch.int32), H.ptr(lut, torch.float32), 0 if lut is None else lut.shape[0], flags,
                                  float(gamma), float(vmin), float(vmax), H.ptr(dst_offset, torch.int64), int(pitch),
                                  0 if colour is None else colour.numel(), H.ptr(out_f32, torch.float32), H.ptr(out_u8, torch.uint8),
                                  H.ptr(out_map, torch.float32), H.ptr(ws), need, H.stream_ptr()), "cvcl_attn_overlay")


def _maps_and_index(images, maps, image_index):
    """-> (maps as [M, h, w], image_of_map int32 [M] or None (map m over image m), the leading shape of the result)."""
    N = images.shape[0]
    if maps.dim() == 3:
        lead, k = tuple(maps.shape[:1]), None
    elif maps.dim() == 4:
        if maps.shape[0] != N:
            raise ValueError(f"[N, k, h, w] maps pair image n with its k maps: {maps.shape[0]} map rows for {N} images")
        lead, k = tuple(maps.shape[:2]), maps.shape[1]
    else:
        raise ValueError(f"maps are [M, h, w], [N, k, h, w] or [N, 1, h, w], got {tuple(maps.shape)}")
    flat = maps.reshape(-1, *maps.shape[-2:]).to(torch.float32).contiguous()
    M = flat.shape[0]
    if image_index is not None:
        if k is not None:
            raise ValueError("image_index goes with [M, h, w] maps; [N, k, h, w] maps are paired by their layout")
        idx = torch.as_tensor(image_index, device=images.device).reshape(-1)
        if idx.numel() != M or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"image_index: one integer per map ({M}), got {tuple(idx.shape)} {idx.dtype}")
        if bool(((idx < 0) | (idx >= N)).any()):
            raise ValueError(f"image_index has entries outside [0, {N})")
        return flat, idx.to(torch.int32).contiguous(), lead
    if k is not None and k > 1:
        return flat, torch.arange(N, dtype=torch.int32, device=images.device).repeat_interleave(k).contiguous(), lead
    if M != N:
        raise ValueError(f"{M} maps for {N} images: give image_index (one image per map) or [N, k, h, w] maps")
    return flat, None, lead


def _overlay_flags(blur, vmin, vmax):
    if (vmin is None) != (vmax is None):
        raise ValueError("vmin and vmax go together")
    return (H.OVERLAY_BLUR if blur else 0) | (0 if vmin is None else H.OVERLAY_HAS_RANGE)


@torch.no_grad()
def overlay_attention_maps(images, maps, image_index=None, blur=True, cmap="viridis", vmin=None, vmax=None, gamma=0.7,
                           mean=IMAGENET_MEAN, std=IMAGENET_STD, out="uint8", return_map=False):
    """getAttMap for a batch, on the device (cvcl_attn_overlay): every map is resized bicubically to the frames' H x W (as
    gradCAM(resize=True) does), blurred (scipy.ndimage.gaussian_filter, sigma = 0.02 max(H, W), mode reflect), normalised to [0, 1] by
    its own min / max, coloured through ``cmap`` and blended into its de-normalised frame with weight x ** gamma.

      images  [N, 3, H, W] fp32, normalised with ``mean`` / ``std`` (undone as img * std + mean)
      maps    [M, h, w] (map m over image m, or over image ``image_index[m]``), [N, k, h, w] (image n with its k maps: the
              ("block", k, .) layouts of gradCAM_pairs and the per-word maps of gradCAM_captions) or [N, 1, h, w]; h <= H, w <= W
      cmap    a matplotlib name (resolved lazily, uploaded once per name and device) or an [n, 3] table: no matplotlib needed
      vmin, vmax  normalise by this range instead and CLAMP x to [0, 1] (getAttMap does not clamp; its x ** 0.7 is NaN below vmin)
      out     "uint8" (floor(clamp(v, 0, 1) * 255 + 0.5)), "float" or "both" (float, uint8): [..., H, W, 3] with the maps' leading shape
      return_map  also return x, the normalised map after the blur, [..., H, W] fp32

    Device tensors only; there is no CPU fallback."""
    if out not in ("uint8", "float", "both"):
        raise ValueError(f"out = {out!r}: 'uint8', 'float' or 'both'")
    if not (torch.is_tensor(images) and torch.is_tensor(maps) and images.is_cuda and maps.is_cuda):
        raise H.CvclError("overlay_attention_maps needs device tensors (got a CPU tensor); there is no CPU fallback")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images are [N, 3, H, W], got {tuple(images.shape)}")
    images = images.to(torch.float32).contiguous()
    flat, index, lead = _maps_and_index(images, maps, image_index)
    flags = _overlay_flags(blur, vmin, vmax)
    M, (Hh, Ww), dev = flat.shape[0], images.shape[2:], images.device
    out_f32 = torch.empty(M, Hh, Ww, 3, dtype=torch.float32, device=dev) if out in ("float", "both") else None
    out_u8 = torch.empty(M, Hh, Ww, 3, dtype=torch.uint8, device=dev) if out in ("uint8", "both") else None
    out_map = torch.empty(M, Hh, Ww, dtype=torch.float32, device=dev) if return_map else None
    _overlay_launch(images, flat, index, device_lut(cmap, dev), flags, gamma, 0.0 if vmin is None else vmin, 0.0 if vmax is None else vmax,
                    mean, std, None, 3 * Ww, out_f32, out_u8, out_map)
    res = [t.view(*lead, *t.shape[1:]) for t in (out_f32, out_u8, out_map) if t is not None]
    return res[0] if len(res) == 1 else tuple(res)


@torch.no_grad()
def attention_grid(images, maps, nrow=4, padding=2, **overlay_kwargs):
    """The reference's attention-map figure (analysis_cvcl/generate_attention_maps.py) as one uint8 [Hc, Wc, 3] device tensor: the K
    frames first, then their K overlays, ``nrow`` per row, laid out as torchvision.utils.make_grid lays out 2 K tiles (``padding``
    pixels of 0 between and around them).  ``images`` [K, 3, H, W], ``maps`` [K, h, w] or [K, 1, h, w]; ``overlay_kwargs``: blur,
    cmap, vmin, vmax, gamma, mean, std of overlay_attention_maps.  Both halves are written straight into the canvas by the overlay
    kernel through its destination table (the frames with weight 0 on the colour): there is no paste pass."""
    unknown = set(overlay_kwargs) - {"blur", "cmap", "vmin", "vmax", "gamma", "mean", "std"}
    if unknown:
        raise TypeError(f"attention_grid: unexpected arguments {sorted(unknown)}")
    if not (torch.is_tensor(images) and torch.is_tensor(maps) and images.is_cuda and maps.is_cuda):
        raise H.CvclError("attention_grid needs device tensors (got a CPU tensor); there is no CPU fallback")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images are [K, 3, H, W], got {tuple(images.shape)}")
    images = images.to(torch.float32).contiguous()
    K, _, Hh, Ww = images.shape
    if maps.dim() == 4 and maps.shape[1] == 1:
        maps = maps[:, 0]
    if maps.dim() != 3 or maps.shape[0] != K:
        raise ValueError(f"maps are [K, h, w] or [K, 1, h, w] with K = {K}, got {tuple(maps.shape)}")
    flat = maps.to(torch.float32).contiguous()
    mean, std = overlay_kwargs.get("mean", IMAGENET_MEAN), overlay_kwargs.get("std", IMAGENET_STD)
    vmin, vmax = overlay_kwargs.get("vmin"), overlay_kwargs.get("vmax")
    flags = _overlay_flags(overlay_kwargs.get("blur", True), vmin, vmax)
    Hc, Wc, origins = grid_geometry(2 * K, Hh, Ww, nrow, padding)
    dev = images.device
    canvas = torch.zeros(Hc, Wc, 3, dtype=torch.uint8, device=dev)
    offsets = torch.tensor([(y * Wc + x) * 3 for y, x in origins], dtype=torch.int64).to(dev)
    _overlay_launch(images, None, None, None, H.OVERLAY_IMAGE_ONLY, 0.0, 0.0, 0.0, mean, std, offsets[:K].contiguous(), 3 * Wc, None, canvas,
                    None)
    _overlay_launch(images, flat, None, device_lut(overlay_kwargs.get("cmap", "viridis"), dev), flags, overlay_kwargs.get("gamma", 0.7),
                    0.0 if vmin is None else vmin, 0.0 if vmax is None else vmax, mean, std, offsets[K:].contiguous(), 3 * Wc, None, canvas,
                    None)
    return canvas


# ---- host-side visualisation (numpy / matplotlib) ------------------------------------------------------------------------

class _Normalize:
    """Per-channel (x - mean) / std over the channel dimension -3 of a tensor or array (torchvision's Normalize arithmetic)."""

    def __init__(self, mean, std):
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)

    def __call__(self, x):
        if torch.is_tensor(x):
            m = torch.tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
            s = torch.tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        else:
            x = np.asarray(x)
            m = np.asarray(self.mean, dtype=x.dtype).reshape(-1, 1, 1)
            s = np.asarray(self.std, dtype=x.dtype).reshape(-1, 1, 1)
        return (x - m) / s


# undoes the ImageNet normalisation of the frames (reference :15-17)
n_inv = _Normalize([-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)], [1.0 / s for s in IMAGENET_STD])


def normalize(x: np.ndarray, vmin=None, vmax=None) -> np.ndarray:
    """Affine map of x onto [0, 1] from [vmin, vmax] (default: x's own range); a constant array maps to 0."""
    lo = x.min() if vmin is None else vmin
    hi = x.max() if vmax is None else vmax
    print(f"normalizing: [vmin, vmax] = [{lo:.6f}, {hi:.6f}] to [0, 1]")
    span = hi - lo
    y = x - lo
    return y / span if span > 0 else y


def preprocess_attn_map(attn_map, shape, interpolation="cubic", blur=False, vmin=None, vmax=None, cmap=None, **kwargs):
    """-> (map at ``shape`` normalised to [0, 1], its RGB colouring under ``cmap`` or None).  Resizing a map of another shape
    needs OpenCV; a map already at ``shape`` (what gradCAM(resize=True) returns) does not."""
    attn_map = np.asarray(attn_map)
    shape = tuple(shape)
    if attn_map.shape != shape:
        import cv2
        flag = getattr(cv2, "INTER_" + interpolation.upper())
        attn_map = cv2.resize(attn_map, (shape[1], shape[0]), interpolation=flag)
    if blur:
        from scipy.ndimage import gaussian_filter
        attn_map = gaussian_filter(attn_map, 0.02 * max(shape))
    attn_map = normalize(attn_map, vmin=vmin, vmax=vmax)
    coloured = None
    if cmap is not None:
        import matplotlib
        coloured = matplotlib.colormaps[cmap](attn_map)[..., :3]
    return attn_map, coloured


def getAttMap(img, attn_map, blur=True, cmap="viridis", **kwargs):
    """Blend of ``img`` [H, W, 3] with the coloured map: weight attn^0.7 on the colour, the rest on the image."""
    attn_map, coloured = preprocess_attn_map(attn_map, img.shape[:2], blur=blur, cmap=cmap, **kwargs)
    weight = (attn_map ** 0.7)[..., None]
    return (1 - weight) * img + weight * coloured


def imshow(ax, img: np.ndarray):
    ax.imshow(img)
    ax.axis("off")


def plot_image(ax, img, attn_map=None, text=None, overlying=True, alpha=0.8, cmap="Greys_r", **kwargs):
    """Draw ``img`` on ``ax`` with the map either laid over it (``overlying``) or blended into it (getAttMap), and a caption."""
    if overlying:
        imshow(ax, img)
        if attn_map is not None:
            attn_map, _ = preprocess_attn_map(attn_map, img.shape[:2], cmap=None, **kwargs)
            ax.imshow(attn_map, alpha=alpha, cmap=cmap)
    else:
        if attn_map is not None:
            img = getAttMap(img, attn_map, cmap=cmap, **kwargs)
        imshow(ax, img)
    if text is not None:
        ax.text(0, 1, text, color="black", backgroundcolor="white")
