"""torch.autograd bridges onto the HIP C ABI for the contrastive head and the trainable projections.

PyTorch owns device memory, autograd bookkeeping and the optimizer; every arithmetic step on the
path is a libcvcl_hip kernel.  Functions raise if handed CPU tensors (no fallback by design).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _hip as H

_F = torch.float32


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


class EmbedMeanPool(torch.autograd.Function):
    """multimodal/multimodal.py:496-503 (reference): embedding gather, sum over L, divide by length."""

    @staticmethod
    def forward(ctx, table, tok, length, want_output: bool):
        B, L = tok.shape
        V, E = table.shape
        ret = torch.empty(B, E, dtype=_F, device=table.device)
        out = torch.empty(B, L, E, dtype=_F, device=table.device) if want_output else None
        H.check(H.lib().cvcl_embed_meanpool_fwd(H.ptr(table, _F), H.ptr(tok, torch.int64), H.ptr(length, torch.int64),
                                               H.ptr(ret), H.ptr(out), B, L, E, V, H.stream_ptr()),
                "cvcl_embed_meanpool_fwd")
        ctx.save_for_backward(tok, length)
        ctx.shape = (V, E)
        ctx.mark_non_differentiable(*([out] if out is not None else []))
        ctx.set_materialize_grads(False)       # (no zero-filled [B, L, E] gradient for the non-differentiable per-word output)
        return ret, out

    @staticmethod
    def backward(ctx, d_ret, _d_out):
        tok, length = ctx.saved_tensors
        if d_ret is None:
            return None, None, None, None
        V, E = ctx.shape
        B, L = tok.shape
        d_table = torch.empty(V, E, dtype=_F, device=d_ret.device)
        H.check(H.lib().cvcl_embed_meanpool_bwd(H.ptr(d_ret.contiguous(), _F), H.ptr(tok), H.ptr(length),
                                               H.ptr(d_table), B, L, E, V, H.stream_ptr()),
                "cvcl_embed_meanpool_bwd")
        return d_table, None, None, None


class L2Normalize(torch.autograd.Function):
    """F.normalize(x, p=2, dim=-1) (reference multimodal/multimodal.py:736,743)."""

    @staticmethod
    def forward(ctx, x, eps: float):
        x = x.contiguous()
        N, E = x.shape
        y = torch.empty_like(x)
        norm = torch.empty(N, dtype=_F, device=x.device)
        H.check(H.lib().cvcl_l2norm_fwd(H.ptr(x, _F), H.ptr(y), H.ptr(norm), N, E, eps, H.stream_ptr()), "cvcl_l2norm_fwd")
        ctx.save_for_backward(y, norm)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        y, norm = ctx.saved_tensors
        N, E = y.shape
        dx = torch.empty_like(y)
        H.check(H.lib().cvcl_l2norm_bwd(H.ptr(y), H.ptr(norm), H.ptr(dy.contiguous(), _F), H.ptr(dx), N, E, ctx.eps,
                                       H.stream_ptr()), "cvcl_l2norm_bwd")
        return dx, None


class SimLogits(torch.autograd.Function):
    """logits_per_image = (img @ txt.T) * exp(neg_log_temp) (reference multimodal/multimodal.py:755,783-787)."""

    @staticmethod
    def forward(ctx, img, txt, neg_log_temp):
        img, txt = img.contiguous(), txt.contiguous()
        Ni, E = img.shape
        Nt = txt.shape[0]
        nlt = neg_log_temp.reshape(1).contiguous()
        logits = torch.empty(Ni, Nt, dtype=_F, device=img.device)
        H.check(H.lib().cvcl_sim_logits_fwd(H.ptr(img, _F), H.ptr(txt, _F), H.ptr(nlt, _F), H.ptr(logits), Ni, Nt, E,
                                           H.stream_ptr()), "cvcl_sim_logits_fwd")
        ctx.save_for_backward(img, txt, nlt, logits)
        ctx.temp_shape = neg_log_temp.shape
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        img, txt, nlt, logits = ctx.saved_tensors
        Ni, E = img.shape
        Nt = txt.shape[0]
        need_i, need_t, need_s = ctx.needs_input_grad
        d_img = torch.empty_like(img) if need_i else None
        d_txt = torch.empty_like(txt) if need_t else None
        d_s = torch.empty(1, dtype=_F, device=img.device) if need_s else None
        nb = H.lib().cvcl_sim_logits_bwd_workspace_bytes(Ni, Nt, E)
        ws = _ws(nb, img.device)
        H.check(H.lib().cvcl_sim_logits_bwd(H.ptr(img), H.ptr(txt), H.ptr(nlt), H.ptr(logits),
                                           H.ptr(d_logits.contiguous(), _F), H.ptr(d_img), H.ptr(d_txt), H.ptr(d_s),
                                           Ni, Nt, E, H.ptr(ws), nb, H.stream_ptr()), "cvcl_sim_logits_bwd")
        return d_img, d_txt, (d_s.reshape(ctx.temp_shape) if need_s else None)


class SpatialMaxLogits(torch.autograd.Function):
    """embedding_type='spatial', sim='max' (reference multimodal/multimodal.py:770-787):
    logits[i][t] = exp(nlt) * sum_l max_p <img[i,p,:], txt[t,l,:]> / len[t].
    img_rows [Bi*HW, E] (per-location features, NHWC order), txt_rows [Bt*L, E] (per-word outputs)."""

    @staticmethod
    def forward(ctx, img_rows, txt_rows, length, neg_log_temp, Bi, HW, Bt, L):
        img_rows, txt_rows = img_rows.contiguous(), txt_rows.contiguous()
        dev = img_rows.device
        nlt = neg_log_temp.reshape(1).contiguous()
        mm = H.gemm(img_rows, txt_rows)                                  # [Bi*HW, Bt*L] match map, fp32
        logits = torch.empty(Bi, Bt, dtype=_F, device=dev)
        arg = torch.empty(Bi, Bt * L, dtype=torch.uint8, device=dev)
        H.check(H.lib().cvcl_spatial_max_fwd(H.ptr(mm), H.ptr(length, torch.int64), H.ptr(nlt, _F), H.ptr(logits), H.ptr(arg),
                                             Bi, HW, Bt, L, H.stream_ptr()), "cvcl_spatial_max_fwd")
        ctx.save_for_backward(img_rows, txt_rows, length, nlt, logits, arg)
        ctx.dims = (Bi, HW, Bt, L)
        ctx.temp_shape = neg_log_temp.shape
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        img_rows, txt_rows, length, nlt, logits, arg = ctx.saved_tensors
        Bi, HW, Bt, L = ctx.dims
        dev = img_rows.device
        E = img_rows.shape[1]
        need_i, need_t, _nl, need_s = ctx.needs_input_grad[:4]
        d_mm = torch.empty(Bi * HW, Bt * L, dtype=_F, device=dev)
        d_s = torch.empty(1, dtype=_F, device=dev) if need_s else None
        s = H.stream_ptr()
        H.check(H.lib().cvcl_spatial_max_bwd(H.ptr(d_logits.contiguous(), _F), H.ptr(arg), H.ptr(length), H.ptr(nlt), H.ptr(logits),
                                             H.ptr(d_mm), H.ptr(d_s), Bi, HW, Bt, L, s), "cvcl_spatial_max_bwd")

        # the operands of both gradient GEMMs are read K-major in place (H.gemm a_trans / w_trans): no transposed copies
        d_img = H.gemm(d_mm, txt_rows, w_trans=True) if need_i else None                    # [Bi*HW, E] = d_mm . txt_rows
        d_txt = H.gemm(d_mm, img_rows, a_trans=True, w_trans=True) if need_t else None      # [Bt*L, E] = d_mm^T . img_rows
        return d_img, d_txt, None, (d_s.reshape(ctx.temp_shape) if need_s else None), None, None, None, None


class TokenCrossEntropy(torch.autograd.Function):
    """F.cross_entropy(logits [R,V], labels [R], ignore_index, reduction='none') (reference multimodal.py:884-889)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        logits = logits.contiguous()
        R, V = logits.shape
        loss = torch.empty(R, dtype=_F, device=logits.device)
        lse = torch.empty(R, dtype=_F, device=logits.device)
        H.check(H.lib().cvcl_token_ce_fwd(H.ptr(logits, _F), H.ptr(labels, torch.int64), H.ptr(loss), H.ptr(lse), R, V, ignore_index,
                                          H.stream_ptr()), "cvcl_token_ce_fwd")
        ctx.save_for_backward(logits, labels, lse)
        ctx.ignore = ignore_index
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        logits, labels, lse = ctx.saved_tensors
        R, V = logits.shape
        d_logits = torch.empty_like(logits)
        H.check(H.lib().cvcl_token_ce_bwd(H.ptr(logits), H.ptr(labels), H.ptr(lse), H.ptr(d_loss.contiguous(), _F), H.ptr(d_logits),
                                          R, V, ctx.ignore, H.stream_ptr()), "cvcl_token_ce_bwd")
        return d_logits, None, None


class LmLossSummaries(torch.autograd.Function):
    """(means [3], counts [3]) of the token-wise LM loss: all non-pad tokens / without <sos> / without <sos>, <eos>
    (reference multimodal_lit.py:284-300)."""

    @staticmethod
    def forward(ctx, loss, labels, pad, sos, eos):
        loss = loss.contiguous()
        R = loss.numel()
        means = torch.empty(3, dtype=_F, device=loss.device)
        counts = torch.empty(3, dtype=_F, device=loss.device)
        H.check(H.lib().cvcl_lm_loss_summaries(H.ptr(loss, _F), H.ptr(labels, torch.int64), None, H.ptr(means), H.ptr(counts), None,
                                               R, pad, sos, eos, H.stream_ptr()), "cvcl_lm_loss_summaries")
        ctx.save_for_backward(labels, counts)
        ctx.meta = (R, pad, sos, eos)
        ctx.mark_non_differentiable(counts)
        return means, counts

    @staticmethod
    def backward(ctx, d_means, _d_counts):
        labels, counts = ctx.saved_tensors
        R, pad, sos, eos = ctx.meta
        d_loss = torch.empty(R, dtype=_F, device=d_means.device)
        H.check(H.lib().cvcl_lm_loss_summaries(None, H.ptr(labels), H.ptr(d_means.contiguous(), _F), None, H.ptr(counts), H.ptr(d_loss),
                                               R, pad, sos, eos, H.stream_ptr()), "cvcl_lm_loss_summaries")
        return d_loss, None, None, None, None


class InfoNCE(torch.autograd.Function):
    """Symmetric InfoNCE + accuracies + entropies (reference multimodal/multimodal.py:801-818)."""

    @staticmethod
    def forward(ctx, logits):
        logits = logits.contiguous()
        N = logits.shape[0]
        assert logits.shape[1] == N, "the contrastive loss needs square logits"
        dev = logits.device
        scalars = torch.empty(5, dtype=_F, device=dev)
        row_lse = torch.empty(N, dtype=_F, device=dev)
        col_lse = torch.empty(N, dtype=_F, device=dev)
        nb = H.lib().cvcl_infonce_workspace_bytes(N)
        ws = _ws(nb, dev)
        H.check(H.lib().cvcl_infonce_fwd(H.ptr(logits, _F), N, H.ptr(scalars), H.ptr(row_lse), H.ptr(col_lse),
                                        H.ptr(ws), nb, H.stream_ptr()), "cvcl_infonce_fwd")
        ctx.save_for_backward(logits, row_lse, col_lse)
        loss = scalars[0].clone()
        metrics = scalars[1:].clone()
        ctx.mark_non_differentiable(metrics)
        ctx.set_materialize_grads(False)
        return loss, metrics

    @staticmethod
    def backward(ctx, d_loss, _d_metrics):
        if d_loss is None:
            return None
        logits, row_lse, col_lse = ctx.saved_tensors
        N = logits.shape[0]
        d_logits = torch.empty_like(logits)
        g = d_loss.reshape(1).to(_F).contiguous()
        H.check(H.lib().cvcl_infonce_bwd(H.ptr(logits), H.ptr(row_lse), H.ptr(col_lse), H.ptr(g), H.ptr(d_logits), N,
                                        H.stream_ptr()), "cvcl_infonce_bwd")
        return d_logits


class LinearF32(torch.autograd.Function):
    """nn.Linear on fp32 operands (fc 2048->E, multimodal/multimodal.py:192; ViT head :190; the text transformer's linears
    :553-573).  ``split`` False: the exact-fp32 MFMA GEMM (the parity mode); True (the bf16 configurations): the same operands on the
    bf16 MFMA with every element split into two bf16 parts -- ~2^-16 relative, ~4x faster (cvcl_gemm_args.f32_split)."""

    @staticmethod
    def forward(ctx, x, weight, bias, split=False):
        x = x.contiguous()
        y = H.gemm(x, weight.contiguous(), bias=bias, split=split)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.split = bool(split)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        return linear_backward(x, weight, dy.contiguous(), (need_x, need_w, need_b and ctx.has_bias), split=ctx.split) + (None,)


def linear_backward(x, weight, dy, needs, split=False):
    """(dx, dw, db) of y = x W^T + b for dy [M, N]: dW[N,K] = dY^T X and dX[M,K] = dY W as GEMMs over operands read K-major in
    place; db = the column sums of dY comes out of the dW GEMM's own operand loads (a_rowsum).  needs = (dx, dw, db) wanted."""
    M, K = x.shape
    N = weight.shape[0]
    need_x, need_w, need_b = needs
    dx = dw = db = None
    if need_b:
        db = torch.empty(N, dtype=_F, device=x.device)
    if need_w:                                       # A' = dY^T: dY is [K' = M][N] in memory; W' = X^T: X is [K' = M][K]
        dw = H.gemm(dy, x, a_trans=True, w_trans=True, a_rowsum=db, split=split)
    elif need_b:
        H.check(H.lib().cvcl_colsum_f32(H.ptr(dy), H.ptr(db), M, N, H.stream_ptr()), "cvcl_colsum_f32")
    if need_x:                                       # W' = W^T: W is [K' = N][K] in memory
        dx = H.gemm(dy, weight.contiguous(), w_trans=True, split=split)
    return dx, dw, db


def token_cross_entropy(logits, labels, ignore_index=0):
    return TokenCrossEntropy.apply(logits, labels, ignore_index)


def lm_loss_summaries(loss, labels, pad=0, sos=2, eos=3):
    return LmLossSummaries.apply(loss, labels, pad, sos, eos)


def spatial_max_logits(img_rows, txt_rows, length, neg_log_temp, Bi, HW, Bt, L):
    return SpatialMaxLogits.apply(img_rows, txt_rows, length, neg_log_temp, Bi, HW, Bt, L)


def embed_meanpool(table, tok, length, want_output=True):
    return EmbedMeanPool.apply(table, tok, length, want_output)


def l2_normalize(x, eps: float = 1e-12):
    return L2Normalize.apply(x, eps)


def sim_logits(img, txt, neg_log_temp):
    return SimLogits.apply(img, txt, neg_log_temp)


def infonce(logits):
    """-> (loss, metrics[4] = image_accuracy, text_accuracy, image_entropy, text_entropy)"""
    return InfoNCE.apply(logits)


def linear_f32(x, weight, bias=None, split=False):
    return LinearF32.apply(x, weight, bias, split)


def _embed_gather(table, tok, pos=None):
    B, L = tok.shape
    V, E = table.shape
    x = torch.empty(B * L, E, dtype=_F, device=table.device)
    H.check(H.lib().cvcl_embed_gather_pos(H.ptr(table.detach(), _F), H.ptr(tok, torch.int64), H.ptr(pos), H.ptr(x), B, L, E, V,
                                         H.stream_ptr()), "cvcl_embed_gather_pos")
    return x


def lstm_initial_state(h0, c0, B, Hd, device):
    """(h, c) [B, H] fp32 for lstm_recurrence to advance in place: copies of ``h0``, ``c0`` (captioning: the image's state), zeros
    when both are absent (reference init_hidden, multimodal.py:671-688)."""
    if (h0 is None) != (c0 is None):
        raise ValueError("LSTM initial state: give both h0 and c0 or neither")
    if h0 is None:
        return torch.zeros(B, Hd, dtype=_F, device=device), torch.zeros(B, Hd, dtype=_F, device=device)
    return tuple(torch.empty(B, Hd, dtype=_F, device=device).copy_(t.detach().reshape(B, Hd)) for t in (h0, c0))


def lstm_recurrence(gx, w_hh, length, state, B, L, save=False):
    """The forward recurrence of the one-layer LSTM, for the eval encoder, the training forward and the per-word Grad-CAM alike.
    ``gx`` [B L, 4H] = x W_ih^T + b_ih + b_hh for all steps (one GEMM, the caller's); per step t one recurrent GEMM
    gates = h W_hh^T + gx[:, t] (the input's gates added through the residual epilogue) and the cell kernel, which advances
    ``state`` = (h, c) [B, H] in place for the sequences still running at t (``length`` [B] int64).  -> out [B, L, H], or with
    ``save`` (cvcl_lstm_cell_train) -> (out, gact [B L, 4H], csave [B L, H], hprev [B L, H]): what BPTT reads."""
    h, c = state
    Hd = w_hh.shape[1]
    dev = gx.device
    lib, s = H.lib(), H.stream_ptr()
    gx = gx.view(B, L, 4 * Hd).unbind(1)                 # step t's rows of gx: row-strided views (H.rows)
    out = torch.empty(B, L, Hd, dtype=_F, device=dev)
    gates = torch.empty(B, 4 * Hd, dtype=_F, device=dev)
    cell = (H.ptr(h, _F), H.ptr(c, _F), H.ptr(out))
    if save:
        gact = torch.zeros(B * L, 4 * Hd, dtype=_F, device=dev)       # (rows of finished sequences stay zero)
        csave = torch.empty(B * L, Hd, dtype=_F, device=dev)
        hprev = torch.empty(B * L, Hd, dtype=_F, device=dev)
        cell += (H.ptr(gact), H.ptr(csave), H.ptr(hprev))
    step, name = (lib.cvcl_lstm_cell_train, "cvcl_lstm_cell_train") if save else (lib.cvcl_lstm_cell, "cvcl_lstm_cell")
    p_gates, p_len = H.ptr(gates), H.ptr(length, torch.int64)
    for t in range(L):
        H.gemm(h, w_hh, residual=gx[t], out=gates, stream=s)
        H.check(step(p_gates, p_len, t, *cell, B, L, Hd, s), name)
    return (out, gact, csave, hprev) if save else out


def lstm_text(table, lstm, tok, length, h0=None, c0=None):
    """Embedding + one-layer uni-directional nn.LSTM over variable-length sequences, eval mode
    (reference multimodal/multimodal.py:513-552).  -> (h at each sequence's last step [B,H], outputs [B,Lmax,H]).
    x W_ih^T for all steps is one GEMM; the steps are lstm_recurrence.  ``h0``, ``c0`` [B, H]: the initial state (captioning,
    init_hidden :671-688); zeros when absent."""
    if lstm.bidirectional or lstm.num_layers != 1:
        raise NotImplementedError("only the one-layer uni-directional LSTM text encoder is on the contrastive path")
    B, L = tok.shape
    with torch.no_grad():
        x = _embed_gather(table, tok)
        bias = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().contiguous()
        gx = H.gemm(x, lstm.weight_ih_l0.detach().contiguous(), bias=bias)             # [B*L, 4H]
        h, c = lstm_initial_state(h0, c0, B, lstm.hidden_size, table.device)
        out = lstm_recurrence(gx, lstm.weight_hh_l0.detach().contiguous(), length, (h, c), B, L)
        lmax = int(length.max())              # pad_packed_sequence trims to the longest sequence (the reference syncs here too)
    return h, out[:, :lmax]


def beam_search_lstm(table, lstm, out_weight, out_bias, batch_size, beam_width, decode_length, alpha, h0=None, c0=None,
                     sos_id=2, eos_id=3, return_steps=False):
    """Beam-search decoding of the one-layer LSTM language model (reference beam_search_decode, multimodal.py:893-960, over
    beam_search.py:232-703) -> (seq [B, K, steps + 1] int64, scores [B, K] f32).  ``h0``, ``c0`` [B, H]: the image-initialised
    state of a captioning model (zeros when absent).  Per step: h W_hh^T (fp32 GEMM), cvcl_lstm_cell_tok (adds row tok of
    G = table W_ih^T + b_ih + b_hh, computed once), the output layer (fp32 GEMM, bias included) and cvcl_beam_step; the stop test
    runs on the device, so the only host sync is the read of the final step count.  ``return_steps``: also return it."""
    if lstm.bidirectional or lstm.num_layers != 1:
        raise NotImplementedError("beam search decodes the one-layer uni-directional LSTM language model")
    if (h0 is None) != (c0 is None):
        raise ValueError("beam_search_lstm: give both h0 and c0 or neither")
    B, K, T = int(batch_size), int(beam_width), int(decode_length)
    V, E = table.shape
    Hd = lstm.hidden_size
    if out_weight.shape != (V, Hd):
        raise ValueError(f"output layer {tuple(out_weight.shape)} does not map H = {Hd} to V = {V}")
    dev = table.device
    lib, s = H.lib(), H.stream_ptr()
    N = B * K
    with torch.no_grad():
        bias = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().contiguous()
        G = H.gemm(table.detach().contiguous(), lstm.weight_ih_l0.detach().contiguous(), bias=bias)      # [V, 4H]
        w_hh = lstm.weight_hh_l0.detach().contiguous()
        w_out = out_weight.detach().contiguous()
        b_out = None if out_bias is None else out_bias.detach().contiguous()
        h = torch.zeros(2, N, Hd, dtype=_F, device=dev)
        c = torch.zeros(2, N, Hd, dtype=_F, device=dev)
        if h0 is not None:                                  # _expand_to_beam_size: every beam of item b starts from b's state
            h[0].copy_(h0.detach().reshape(B, 1, Hd).expand(B, K, Hd).reshape(N, Hd))
            c[0].copy_(c0.detach().reshape(B, 1, Hd).expand(B, K, Hd).reshape(N, Hd))
        alive_lp = torch.full((2, B, K), -float("inf"), dtype=_F, device=dev)
        alive_lp[0, :, 0] = 0.
        fin = torch.full((2, B, K), -1e7, dtype=_F, device=dev)                    # beam_search.py INF = 1e7
        alive_seq = torch.zeros(B, K, T + 1, dtype=torch.int64, device=dev)
        alive_seq[:, :, 0] = sos_id
        fin_seq = torch.zeros(B, K, T + 1, dtype=torch.int64, device=dev)
        flags = torch.zeros(B, K, dtype=torch.int32, device=dev)
        tok = torch.full((N,), sos_id, dtype=torch.int64, device=dev)
        steps = torch.full((1,), T, dtype=torch.int32, device=dev)
        gates = torch.empty(N, 4 * Hd, dtype=_F, device=dev)
        logits = torch.empty(N, V, dtype=_F, device=dev)
        for i in range(T):
            a, b = i & 1, (i + 1) & 1
            H.gemm(h[a], w_hh, out=gates)
            H.check(lib.cvcl_lstm_cell_tok(H.ptr(gates), H.ptr(G), H.ptr(tok), V, H.ptr(h[a]), H.ptr(c[a]), N, Hd, s),
                    "cvcl_lstm_cell_tok")
            H.gemm(h[a], w_out, out=logits, bias=b_out)
            H.check(lib.cvcl_beam_step(H.ptr(logits), B, K, V, T, i, float(alpha), int(eos_id), H.ptr(alive_lp[a]),
                                       H.ptr(alive_lp[b]), H.ptr(fin[a]), H.ptr(fin[b]), H.ptr(alive_seq), H.ptr(fin_seq),
                                       H.ptr(flags), H.ptr(h[a]), H.ptr(c[a]), H.ptr(h[b]), H.ptr(c[b]), Hd, H.ptr(tok),
                                       H.ptr(steps), s), "cvcl_beam_step")
        f = T & 1
        out_seq = torch.empty(B, K, T + 1, dtype=torch.int64, device=dev)
        out_scores = torch.empty(B, K, dtype=_F, device=dev)
        H.check(lib.cvcl_beam_finalize(B, K, T, H.ptr(alive_seq), H.ptr(alive_lp[f]), H.ptr(fin_seq), H.ptr(fin[f]), H.ptr(flags),
                                       H.ptr(out_seq), H.ptr(out_scores), s), "cvcl_beam_finalize")
        n = int(steps.item())                               # the one host sync: the reference's final loop index
    seq = out_seq[:, :, :n + 1].contiguous()
    return (seq, out_scores, n) if return_steps else (seq, out_scores)


def transformer_text(table, layer, pos_embed, tok, length):
    """Embedding (+pos) + one post-norm nn.TransformerEncoderLayer with key-padding mask + sum/len, eval mode
    (reference multimodal/multimodal.py:553-573).  -> (ret [B,E], outputs [B,L,E])."""
    B, L = tok.shape
    E = table.shape[1]
    nh = layer.self_attn.num_heads
    lib, s = H.lib(), H.stream_ptr()
    with torch.no_grad():
        pos = None if pos_embed is None else pos_embed.detach()[:L, 0].contiguous().float()
        x = _embed_gather(table, tok, pos)                                              # [B*L, E]
        sa = layer.self_attn
        qkv = H.gemm(x, sa.in_proj_weight.detach().contiguous(), bias=sa.in_proj_bias.detach().contiguous())
        att = torch.empty(B * L, E, dtype=_F, device=x.device)
        H.check(lib.cvcl_attention(H.F32, H.ptr(qkv), H.ptr(tok, torch.int64), H.ptr(att), B, L, nh, E // nh,
                                   float((E // nh) ** -0.5), s), "cvcl_attention")
        y = H.gemm(att, sa.out_proj.weight.detach().contiguous(), bias=sa.out_proj.bias.detach().contiguous(), residual=x)
        h1 = torch.empty_like(y)
        H.check(lib.cvcl_layernorm(H.F32, H.ptr(y), E, H.ptr(layer.norm1.weight.detach()), H.ptr(layer.norm1.bias.detach()),
                                   layer.norm1.eps, H.ptr(h1), 1, B * L, E, s), "cvcl_layernorm")
        f = H.gemm(h1, layer.linear1.weight.detach().contiguous(), bias=layer.linear1.bias.detach().contiguous(), act=H.ACT_RELU)
        y2 = H.gemm(f, layer.linear2.weight.detach().contiguous(), bias=layer.linear2.bias.detach().contiguous(), residual=h1)
        h2 = torch.empty_like(y2)
        H.check(lib.cvcl_layernorm(H.F32, H.ptr(y2), E, H.ptr(layer.norm2.weight.detach()), H.ptr(layer.norm2.bias.detach()),
                                   layer.norm2.eps, H.ptr(h2), 1, B * L, E, s), "cvcl_layernorm")
        ret = torch.empty(B, E, dtype=_F, device=x.device)
        H.check(lib.cvcl_seq_sum_div(H.ptr(h2), H.ptr(length, torch.int64), H.ptr(ret), B, L, E, s), "cvcl_seq_sum_div")
    return ret, h2.view(B, L, E)


def token_items_accumulate(outputs, loss, seg_ptr, rows, slot, vector, loss_sum, cnt):
    """The per-key sums of one batch (reference analysis_tools/processing.py:326-331) added in place to the running tables
    ``vector`` [K, H] f32, ``loss_sum`` [K] f64, ``cnt`` [K] int64.  ``outputs`` [N, H] f32 and ``loss`` [N] f32 are the batch's
    positions; ``seg_ptr`` [S + 1], ``rows`` [seg_ptr[-1]], ``slot`` [S] (int32, on the device) the CSR over the keys present:
    cvcl_token_items_accumulate adds every segment's rows one by one in ``rows`` order.  The caller guarantees that the entries
    of ``slot`` are distinct (processing.build_batch_csr does): nothing checks it, and two segments of one slot would race on
    the key's table row."""
    N, Hd = outputs.shape
    S = slot.numel()
    if seg_ptr.numel() != S + 1 or loss.numel() != N or vector.dim() != 2 or vector.shape[1] != Hd or \
            loss_sum.numel() != vector.shape[0] or cnt.numel() != vector.shape[0]:
        raise ValueError("token_items_accumulate: shapes do not fit together")
    i32 = torch.int32
    H.check(H.lib().cvcl_token_items_accumulate(
        H.ptr(outputs, _F), H.ptr(loss, _F), N, Hd, H.ptr(seg_ptr, i32), H.ptr(rows, i32), H.ptr(slot, i32), S, rows.numel(),
        H.ptr(vector, _F), H.ptr(loss_sum, torch.float64), H.ptr(cnt, torch.int64), vector.shape[0], H.stream_ptr()),
        "cvcl_token_items_accumulate")


def token_topk(logits, labels, k, pad_id=0, want_probs=False):
    """Softmax over the vocabulary and its ``k`` best entries in one pass (reference processing.py:352, utils.py:142) ->
    (top_prob [R, k] f32, top_idx [R, k] int64, label_prob [R] f32, probs [R, V] f32 or None).  Ordered by (probability desc,
    index asc); ``label_prob`` is 0 where the label is ``pad_id``."""
    R, V = logits.shape
    dev = logits.device
    if labels.numel() != R:
        raise ValueError("token_topk: one label per row")
    H.ptr(logits, _F)                                       # refuses CPU tensors before anything is allocated beside them
    top_prob = torch.empty(R, k, dtype=_F, device=dev)
    top_idx = torch.empty(R, k, dtype=torch.int64, device=dev)
    label_prob = torch.empty(R, dtype=_F, device=dev)
    probs = torch.empty(R, V, dtype=_F, device=dev) if want_probs else None
    H.check(H.lib().cvcl_token_topk(H.ptr(logits, _F), H.ptr(labels, torch.int64), R, V, int(k), int(pad_id), H.ptr(top_prob),
                                    H.ptr(top_idx), H.ptr(label_prob), H.ptr(probs), H.stream_ptr()), "cvcl_token_topk")
    return top_prob, top_idx, label_prob, probs


def ngram_keys(y, y_len, N, vocab_size):
    """The packed (n + 1)-grams NGramModel.update counts (reference ngram.py:28-36), every order in one launch -> (keys [N, B, L]
    int64 with CVCL_NGRAM_SENTINEL where nothing is counted, bad [1] int32: the ids outside [0, vocab_size) inside the lengths).
    ``y`` [B, L] and ``y_len`` [B] are contiguous int64 device tensors."""
    B, L = y.shape
    if y_len.numel() != B:
        raise ValueError("ngram_keys: one length per utterance")
    H.ptr(y, torch.int64)                                   # refuses CPU tensors before anything is allocated beside them
    keys = torch.empty(N, B, L, dtype=torch.int64, device=y.device)
    bad = torch.empty(1, dtype=torch.int32, device=y.device)
    H.check(H.lib().cvcl_ngram_keys(H.ptr(y, torch.int64), H.ptr(y_len, torch.int64), B, L, int(N), int(vocab_size), H.ptr(keys),
                                    H.ptr(bad), H.stream_ptr()), "cvcl_ngram_keys")
    return keys, bad


def _ngram_score(entry, tables, N, vocab_size, log_alpha, log_1m_alpha, y, y_len, out):
    gram_key, gram_cnt, gram_off, ctx_key, ctx_tot, ctx_off = tables
    if len(gram_off) != N + 1 or len(ctx_off) != N + 1:
        raise ValueError(f"{entry}: N + 1 offsets per table")
    B, L = y.shape
    if y_len.numel() != B:
        raise ValueError(f"{entry}: one length per utterance")
    i64 = torch.int64
    bad = torch.empty(1, dtype=torch.int32, device=y.device)
    H.check(getattr(H.lib(), entry)(
        H.ptr(gram_key, i64), H.ptr(gram_cnt, i64), (C.c_int64 * (N + 1))(*gram_off), gram_key.numel(), H.ptr(ctx_key, i64),
        H.ptr(ctx_tot, i64), (C.c_int64 * (N + 1))(*ctx_off), ctx_key.numel(), int(N), int(vocab_size), float(log_alpha),
        float(log_1m_alpha), H.ptr(y, i64), H.ptr(y_len, i64), B, L, H.ptr(out, _F), H.ptr(bad), H.stream_ptr()), entry)
    return out, bad


def ngram_ce_loss(tables, N, vocab_size, log_alpha, log_1m_alpha, y, y_len, out=None):
    """The token losses of the back-off n-gram model (reference ngram.py:54-74) -> (loss [B, L - 1] f32, zeros outside the
    utterances; bad [1] int32).  ``tables`` = (gram_key, gram_cnt, gram_off, ctx_key, ctx_tot, ctx_off): the sorted tables of all
    orders concatenated (int64, on the device) and their N + 1 offsets each (host ints), as cvcl_hip.h "N-gram baseline" lays
    them out.  ``out``: the [B, L - 1] f32 buffer to write (every element is written)."""
    B, L = y.shape
    H.ptr(y, torch.int64)
    loss = torch.empty(B, L - 1, dtype=_F, device=y.device) if out is None else out
    if tuple(loss.shape) != (B, L - 1):
        raise ValueError("ngram_ce_loss: out must be [B, L - 1]")
    return _ngram_score("cvcl_ngram_ce_loss", tables, N, vocab_size, log_alpha, log_1m_alpha, y, y_len, loss)


def ngram_probs(tables, N, vocab_size, log_alpha, log_1m_alpha, y, y_len, out=None):
    """exp of the same back-off score for every candidate word -> (probs [B, L - 1, vocab_size] f32, zero rows outside the
    utterances; bad [1] int32).  Not normalised over the words."""
    B, L = y.shape
    H.ptr(y, torch.int64)
    probs = torch.empty(B, L - 1, vocab_size, dtype=_F, device=y.device) if out is None else out
    if tuple(probs.shape) != (B, L - 1, vocab_size):
        raise ValueError("ngram_probs: out must be [B, L - 1, vocab_size]")
    return _ngram_score("cvcl_ngram_probs", tables, N, vocab_size, log_alpha, log_1m_alpha, y, y_len, probs)


def bleu_from_totals(totals):
    """The eight closing lines of pycocoevalcap's BleuScorer.compute_score (option "closest") on the corpus sums of
    cvcl_caption_bleu_rouge's ten statistics, in float64 on the host -> [BLEU_1, .., BLEU_4]."""
    testlen, reflen, guess, correct = totals[0], totals[1], totals[2:6], totals[6:10]
    tiny, small = 1e-15, 1e-9
    ratio = (testlen + tiny) / (reflen + small)
    out, b = [], 1.0
    for k in range(4):
        b *= (correct[k] + tiny) / (guess[k] + small)
        score = b ** (1.0 / (k + 1))
        out.append(score * math.exp(1 - 1 / ratio) if ratio < 1 else score)
    return out


def caption_scores(hyp, hyp_len, ref, ref_len, ref_off, vocab_size):
    """BLEU-1..4, ROUGE-L and CIDEr of N hypotheses against their references (include/cvcl_hip.h "Caption scores") ->
    (scores, arrays).  ``hyp`` [N, Lh], ``hyp_len`` [N], ``ref`` [R, Lr], ``ref_len`` [R] and ``ref_off`` [N + 1] are contiguous
    int64 device tensors of ids in [0, vocab_size): example i owns the references ref_off[i] .. ref_off[i + 1].
    ``scores``: {"BLEU_1", .., "BLEU_4", "ROUGE_L", "CIDEr": float}, the corpus numbers.  ``arrays``: "stats" [N, 10] int64,
    "rouge" and "cider" [N] f64 per example, and "df": per order n = 1..4 the sorted packed n-grams of the references and the number
    of examples that hold each.  Sorting and run-length counting the keys, the two means and BLEU's closing lines are plumbing."""
    N, Lh = hyp.shape
    R, Lr = ref.shape
    if hyp_len.numel() != N or ref_len.numel() != R or ref_off.numel() != N + 1:
        raise ValueError("caption_scores: one length per sentence and N + 1 reference offsets")
    i64, f64, dev = torch.int64, torch.float64, hyp.device
    corpus = (H.ptr(ref, i64), H.ptr(ref_len, i64), R, Lr)          # (refuses CPU tensors before anything is allocated beside them)
    hyps = (H.ptr(hyp, i64), H.ptr(hyp_len, i64), N, Lh)
    offsets = ((C.c_int64 * (N + 1))(*ref_off.tolist()), H.ptr(ref_off, i64), int(vocab_size))
    lib, stream = H.lib(), H.stream_ptr()
    stats = torch.empty(N, 10, dtype=i64, device=dev)
    rouge, cider = torch.empty(N, dtype=f64, device=dev), torch.empty(N, dtype=f64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    H.check(lib.cvcl_caption_bleu_rouge(*hyps, *corpus, *offsets, H.ptr(stats), H.ptr(rouge), H.ptr(bad), stream), "cvcl_caption_bleu_rouge")
    keys = torch.empty(H.CAPTION_ORDERS, R, Lr, dtype=i64, device=dev)
    H.check(lib.cvcl_caption_ref_keys(*corpus[:2], N, R, Lr, *offsets, H.ptr(keys), stream), "cvcl_caption_ref_keys")
    if int(bad):
        raise ValueError(f"caption_scores: {int(bad)} token ids outside [0, {vocab_size})")
    df = []
    for n in range(H.CAPTION_ORDERS):
        k, cnt = torch.unique_consecutive(torch.sort(keys[n].reshape(-1)).values, return_counts=True)
        first = int(k[0] == H.CAPTION_SENTINEL)                     # the sentinel is negative: it sorts in front of every key
        df.append((k[first:], cnt[first:]))
    df_off = [0]
    for k, _ in df:
        df_off.append(df_off[-1] + k.numel())
    df_key, df_cnt = torch.cat([k for k, _ in df]), torch.cat([c for _, c in df])
    H.check(lib.cvcl_caption_cider(*hyps, *corpus, *offsets, H.ptr(df_key, i64), H.ptr(df_cnt, i64),
                                   (C.c_int64 * (H.CAPTION_ORDERS + 1))(*df_off), df_off[-1], H.ptr(cider), stream), "cvcl_caption_cider")
    scores = dict(zip(("BLEU_1", "BLEU_2", "BLEU_3", "BLEU_4"), bleu_from_totals(stats.sum(0).tolist())))
    scores["ROUGE_L"] = float(rouge.sum()) / N
    scores["CIDEr"] = float(cider.sum()) / N
    return scores, {"stats": stats, "rouge": rouge, "cider": cider, "df": df}
