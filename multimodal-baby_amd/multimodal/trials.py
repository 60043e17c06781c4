"""Forced-choice evaluation from tables: every distinct frame and every category word is encoded once, and all trials are scored
from an index table in one launch of ``cvcl_trial_scores`` (csrc/trials.hip).

The reference's loop (eval.py:196-232) runs ``model(img, label, label_len)`` per trial.  The object-category evaluation draws 5
trials per image with 3 foil images each from the same folders, so that loop passes every file through the image encoder about
20 times and every one-word label thousands of times.  Eval-mode encoders are per sample: the features of a frame do not depend
on the trial it appears in, and a trial's logits are dot products between rows of two feature tables (up to the rounding of the
encoders' batch-dependent GEMM routes, DESIGN.md section 9 "Object-category evaluation").

Which models this covers (``table_route``): flat embeddings; CLIP; spatial embeddings under ``sim == "mean"``, whose logit is the
dot product of the pooled rows (``SeqSumDiv``, as ``MultiModalModel.forward`` pools them).  ``sim == "max"`` is a maximum over
locations per word and has no table form: eval.py keeps the per-trial path for it."""
from __future__ import annotations

import numpy as np
import torch

from . import _hip as H
from . import ops


def _is_clip(model):
    return hasattr(model, "logit_scale") and hasattr(model, "visual")


def _core(model):
    """the MultiModalModel of a MultiModalLitModel (or the model itself)"""
    return getattr(model, "model", model)


def table_route(model):
    """Can the trials of ``model`` be scored from feature tables?  -> None if so, else the reason as text."""
    if _is_clip(model):
        return None
    m = _core(model)
    if getattr(m, "embedding_type", "flat") == "spatial" and getattr(m, "sim", "mean") != "mean":
        return f"spatial embeddings with sim == {m.sim!r} take a maximum over locations per word: there is no feature table to index"
    return None


def log_scale_of(model, device):
    """The device scalar the logits are scaled by the exponential of: logit_neg_log_temperature, or CLIP's logit_scale."""
    if _is_clip(model):
        return model.logit_scale.detach().to(device=device, dtype=torch.float32).contiguous()
    return _core(model)._temperature_on(device).detach().to(dtype=torch.float32).contiguous()


@torch.no_grad()
def _image_rows(model, frames):
    """[B, 3, H, W] -> [B, D] fp32: the rows ``forward`` multiplies (normalised as encode_image does; spatial maps pooled)"""
    if _is_clip(model):
        return ops.l2_normalize(model.encode_image(frames)).float()
    f = _core(model).encode_image(frames)[0]
    if f.dim() == 4:                                       # spatial, sim == "mean": the mean location (MultiModalModel.forward)
        from .text_train import SeqSumDiv
        B, E, Hh, Ww = f.shape
        rows = f.permute(0, 2, 3, 1).reshape(B * Hh * Ww, E).float()
        hw = torch.full((B,), Hh * Ww, dtype=torch.int64, device=f.device)
        return SeqSumDiv.apply(rows, hw, B, Hh * Ww)
    return f.float()


@torch.no_grad()
def encode_frames_once(model, datamodule, files, batch=256, eval_type=None):
    """The features of ``files`` (paths), each decoded, preprocessed (``datamodule.load_frames``: host decode, the dataset's device
    transform) and encoded once, in passes of ``batch`` frames -> [len(files), D] fp32 on the device, normalised as the model's
    ``encode_image`` does."""
    route = table_route(model)
    if route:
        raise H.CvclError(f"encode_frames_once: {route}")
    batch = max(1, int(batch))
    out = [_image_rows(model, datamodule.load_frames(files[s:s + batch], eval_type)) for s in range(0, len(files), batch)]
    if not out:
        raise H.CvclError("encode_frames_once: no files")
    return torch.cat(out, 0).contiguous()


@torch.no_grad()
def encode_words_once(model, word_rows, lens=None):
    """The features of the label rows ``word_rows`` [C, L] int64 (``lens`` [C]; CLIP: [C, 77] token rows, no lengths) -> [C, D]
    fp32 on the device, as ``forward`` multiplies them."""
    route = table_route(model)
    if route:
        raise H.CvclError(f"encode_words_once: {route}")
    if _is_clip(model):
        dev = model.logit_scale.device
        return ops.l2_normalize(model.encode_text(word_rows.to(dev))).float().contiguous()
    m = _core(model)
    dev = next(m.parameters()).device
    rows, lens = word_rows.to(dev), torch.as_tensor(lens).long().to(dev)
    f = m.encode_text(rows, lens)[0]
    if f.dim() == 3:                                       # spatial, sim == "mean": sum of the words / length
        from .text_train import SeqSumDiv
        C, L, E = f.shape
        return SeqSumDiv.apply(f.reshape(C * L, E).float(), lens, C, L)
    return f.float().contiguous()


def _indices(idx, device, what):
    t = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx)
    if t.dtype not in (torch.int32, torch.int64):
        raise H.CvclError(f"score_trials: {what} must hold integers, got {t.dtype}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def score_trials(query, cand, q_idx, c_idx, log_scale=None, return_logits=False):
    """``cvcl_trial_scores``: query [Nq, D], cand [Nc, D] fp32 device rows (a row stride above D is read in place), q_idx [T],
    c_idx [T, n] integers, log_scale a device scalar or None -> (probs [T, n] fp32, pred [T] int32) on the HOST, fetched in one
    device-to-host copy for all trials (``return_logits``: the device tensor of the logits as a third value).  A trial with an index
    outside its table has NaN probabilities and pred -1.  CPU tensors are refused: there is no fallback."""
    for name, t in (("query", query), ("cand", cand)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise H.CvclError(f"score_trials({name}): the trial scorer needs device tensors (got "
                              f"{type(t).__name__ if not torch.is_tensor(t) else 'a CPU tensor'}); there is no CPU fallback")
        if t.dim() != 2 or t.dtype != torch.float32:
            raise H.CvclError(f"score_trials({name}): expected [N, D] fp32 rows, got {tuple(t.shape)} {t.dtype}")
    q = query if H.row_strided(query) else query.contiguous()
    c = cand if H.row_strided(cand) else cand.contiguous()
    if q.shape[1] != c.shape[1]:
        raise H.CvclError(f"score_trials: query rows are {q.shape[1]} wide, cand rows {c.shape[1]}")
    qi, ci = _indices(q_idx, q.device, "q_idx"), _indices(c_idx, q.device, "c_idx")
    if qi.dim() != 1 or ci.dim() != 2 or ci.shape[0] != qi.shape[0]:
        raise H.CvclError(f"score_trials: expected q_idx [T] and c_idx [T, n], got {tuple(qi.shape)} and {tuple(ci.shape)}")
    T, n = ci.shape
    if log_scale is not None:
        if not torch.is_tensor(log_scale) or not log_scale.is_cuda or log_scale.numel() != 1 or log_scale.dtype != torch.float32:
            raise H.CvclError("score_trials: log_scale must be a one-element fp32 device tensor (or None)")
        log_scale = log_scale.detach().contiguous()
    # probs [T, n] fp32 and pred [T] int32 in one buffer of 4-byte words: one copy to the host
    out = torch.empty(T * (n + 1), dtype=torch.float32, device=q.device)
    probs, pred = out[:T * n].view(T, n), out[T * n:].view(torch.int32)
    logits = torch.empty(T, n, dtype=torch.float32, device=q.device) if return_logits else None
    if T:                                                  # (no trials: nothing to enqueue, and an empty tensor has no pointer)
        with torch.cuda.device(q.device):
            H.check(H.lib().cvcl_trial_scores(*H.rows(q), q.shape[0], *H.rows(c), c.shape[0], q.shape[1], H.ptr(qi), H.ptr(ci), T, n,
                                              H.ptr(log_scale), H.ptr(logits), H.ptr(probs), H.ptr(pred), H.stream_ptr()),
                    "cvcl_trial_scores")
    host = out.cpu()
    res = (host[:T * n].view(T, n), host[T * n:].view(torch.int32))
    return res + (logits,) if return_logits else res


@torch.no_grad()
def evaluate_trial_table(model, datamodule, eval_type, use_kitty_label=False, frame_batch=256):
    """All trials of an ``ObjectCategoriesDataModule`` (after ``setup``) -> [(soft-max list, pred)] in the metadata's order, the
    values eval.py's per-trial loop appends: frames and words encoded once, one scoring launch, one copy to the host."""
    table = datamodule.trial_table(eval_type, use_kitty_label)
    frames = encode_frames_once(model, datamodule, datamodule.frame_files, frame_batch, eval_type)
    words = encode_words_once(model, table["word_rows"], table["word_lens"])
    query, cand = (words, frames) if eval_type == "image" else (frames, words)
    probs, pred = score_trials(query, cand, table["q_idx"], table["c_idx"], log_scale_of(model, frames.device))
    return list(zip(probs.numpy().tolist(), (int(p) for p in pred)))
