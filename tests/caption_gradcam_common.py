"""Shared by the per-word Grad-CAM tests: the formula-filled toy weights of tests/golden/caption_gradcam.npz (as
tools/gen_golden_caption_gradcam.py fills them), the CPU reference arithmetic (torch.nn.LSTM / F.cross_entropy / F.normalize
autograd, any dtype) and the bound the issue sets."""
import argparse
import contextlib
import io

import torch
import torch.nn.functional as F

from gen_golden import formula_fill_, small_vocab

V, E, C, HW, B, L = 50, 32, 48, 7, 6, 9
TE_KEYS = ("connector.bias", "connector.weight", "embedding.weight", "lstm.bias_hh_l0", "lstm.bias_ih_l0", "lstm.weight_hh_l0",
           "lstm.weight_ih_l0")                                               # sorted(state_dict) of the captioning LSTM text encoder
TE_SCALE = {"embedding.weight": 0.8, "connector.weight": 0.6, "connector.bias": 0.4}


def bound(ref32_dev):
    """max|got - want| / max|want| allowed: 10 x the reference's own fp32-vs-float64 distance, at least 1e-5 (the contraction's
    bound, test_gradcam_gpu.py), at most 2e-4 (this gradient chain's bound, test_captioning_train_gpu.py)."""
    return min(2e-4, max(1e-5, 10.0 * float(ref32_dev)))


def err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def toy_weights():
    shapes = {"connector.bias": (2 * E,), "connector.weight": (2 * E, E), "embedding.weight": (V, E), "lstm.bias_hh_l0": (4 * E,),
              "lstm.bias_ih_l0": (4 * E,), "lstm.weight_hh_l0": (4 * E, E), "lstm.weight_ih_l0": (4 * E, E)}
    w = {k: formula_fill_(torch.empty(shapes[k]), i, TE_SCALE.get(k, 0.5)) for i, k in enumerate(TE_KEYS)}
    w["out_bias"] = formula_fill_(torch.empty(V), 98, 0.5)
    w["fc.weight"] = formula_fill_(torch.empty(E, C), 200, 0.3)
    w["fc.bias"] = formula_fill_(torch.empty(E), 201, 0.2)
    return w


def weights_of(language_model):
    """The same dictionary from a LanguageModel of this repository (tied output layer)."""
    te = language_model.text_encoder
    w = {k: v.detach().cpu() for k, v in te.state_dict().items() if k in TE_KEYS}
    w["out_bias"] = language_model.output_layer.bias.detach().cpu()
    return w


def lm_args(E_, normalize=False):
    return argparse.Namespace(
        embedding_type="flat", embedding_dim=E_, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False, vit_dino=False,
        finetune_cnn=False, text_encoder="lstm", captioning=True, attention=False, attention_gate=False, crange=1, dropout_i=0.0,
        dropout_o=0.0, pos_embed_type="no_pos_embed", normalize_features=normalize, sim="max", temperature=0.07, fix_temperature=False,
        tie=True, bias=True, lr=1e-4, weight_decay=0.1, lambda_mm=0.5, lambda_lm=0.5, lambda_ar=0.0, optimize_unused=True,
        lr_scheduler=False, optimizer=torch.optim.AdamW)


def toy_language_model(dev):
    from multimodal.multimodal import LanguageModel, TextEncoder
    args = lm_args(E)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(small_vocab(V), 2048, args)
        lm = LanguageModel(te, args)
    w = toy_weights()
    te.load_state_dict({k: w[k] for k in TE_KEYS})
    with torch.no_grad():
        lm.output_layer.bias.copy_(w["out_bias"])
    return lm.to(dev).eval(), w


def reference_grads(f, w, y, normalize, dtype=torch.float64):
    """g[b, p] = d loss[b, p] / d f[b] on the CPU in ``dtype``: F.normalize -> connector -> torch.nn.LSTM from (h0, c0) ->
    tied output layer -> F.cross_entropy(ignore_index=<pad>, reduction none), one autograd pass per position (captions are
    independent, so d sum_b loss[b, p] / d f has the per-caption gradients in its rows).  The LSTM runs unpacked: a position inside
    a caption never sees what follows it, and positions whose label is <pad> have zero loss."""
    w = {k: v.detach().cpu().to(dtype) for k, v in w.items()}
    Hd = w["lstm.weight_hh_l0"].shape[1]
    fr = f.detach().cpu().to(dtype).clone().requires_grad_(True)
    n = F.normalize(fr, p=2, dim=1) if normalize else fr
    st = n @ w["connector.weight"].t() + w["connector.bias"]
    lstm = torch.nn.LSTM(w["embedding.weight"].shape[1], Hd, batch_first=True).to(dtype)
    with torch.no_grad():
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(lstm, k).copy_(w["lstm." + k])
    for p in lstm.parameters():
        p.requires_grad_(False)
    y = y.detach().cpu().long()
    x = w["embedding.weight"][y[:, :-1]]
    out, _ = lstm(x, (st[:, :Hd].contiguous()[None], st[:, Hd:].contiguous()[None]))
    logits = out @ w["embedding.weight"].t() + w["out_bias"]
    Bn, K = y.shape[0], y.shape[1] - 1
    loss = F.cross_entropy(logits.reshape(Bn * K, -1), y[:, 1:].reshape(-1), ignore_index=0, reduction="none").view(Bn, K)
    g = torch.zeros(Bn, K, fr.shape[1], dtype=dtype)
    for p in range(K):
        g[:, p] = torch.autograd.grad(loss[:, p].sum(), fr, retain_graph=True)[0]
    return g


def reference_cams(A, g, fc_weight):
    """relu(sum_c alpha_c A[b, c]), alpha = -(g[b, p] @ W_fc) / hw, in g's dtype."""
    A = A.detach().cpu().to(g.dtype)
    alpha = -(g @ fc_weight.detach().cpu().to(g.dtype)) / (A.shape[2] * A.shape[3])
    return torch.einsum("bpc,bchw->bphw", alpha, A).clamp(min=0)


def reference(A, f, fc_weight, w, y, normalize):
    """-> (g64, cams64, ref32_dev of the cams, ref32_dev of g): the float64 values and the distance of the same arithmetic in fp32."""
    g64 = reference_grads(f, w, y, normalize)
    cam64 = reference_cams(A, g64, fc_weight)
    g32 = reference_grads(f, w, y, normalize, torch.float32)
    cam32 = reference_cams(A, g32, fc_weight)
    return g64, cam64, err(cam32, cam64), err(g32, g64)
