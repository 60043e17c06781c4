"""Shared by the word-statistics tests: the fixture's data, the formula-filled toy models of tests/golden/word_statistics.npz (as
tools/gen_golden_word_statistics.py fills them), a float64 restatement of the reference's per-word arithmetic (torch.nn.LSTM /
F.cross_entropy on the CPU, sums in visiting order) and the bounds the checks use."""
import argparse
import contextlib
import io

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden
from gen_golden import formula_fill_, small_vocab

V, E = 50, 32
N_BATCHES = 2
SCALE = {"embedding.weight": 0.8, "connector.weight": 0.6, "connector.bias": 0.4}


def softmax_bound(logits):
    """-> (bound, measured): max|got - want| / max|want| allowed for probabilities of these logits against float64: 10 x the
    distance of torch's own fp32 CPU softmax from float64 on the same logits, at least 1e-6 (the rule of caption_gradcam_common.bound)."""
    lg = logits.detach().cpu()
    p64 = lg.double().softmax(-1)
    measured = float((lg.float().softmax(-1).double() - p64).abs().max() / p64.abs().max())
    return max(1e-6, 10.0 * measured), measured


def err(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def fixture():
    z = load_golden("word_statistics")
    batches = [(z[f"x{i}"], z[f"y{i}"], z[f"y_len{i}"], None) for i in range(N_BATCHES)]
    pos_tags = [s.split() for s in z["pos_tags"].tolist()]
    return z, batches, pos_tags


def toy_weights(captioning):
    """sorted(state_dict) of the reference's LSTM text encoder, filled by index as tools/gen_golden_captioning.build does."""
    H4 = 4 * E
    shapes = {"embedding.weight": (V, E), "lstm.bias_hh_l0": (H4,), "lstm.bias_ih_l0": (H4,), "lstm.weight_hh_l0": (H4, E),
              "lstm.weight_ih_l0": (H4, E)}
    if captioning:
        shapes.update({"connector.bias": (2 * E,), "connector.weight": (2 * E, E)})
    w = {k: formula_fill_(torch.empty(shapes[k]), i, SCALE.get(k, 0.5)) for i, k in enumerate(sorted(shapes))}
    w["out_bias"] = formula_fill_(torch.empty(V), 98, 0.5)
    return w


class StubLit(torch.nn.Module):
    """What analysis_tools.processing touches of a MultiModalLitModel; the image encoder is the identity on flat features."""

    def __init__(self, language_model):
        super().__init__()
        self.language_model = language_model
        self.text_encoder = language_model.text_encoder

    def calculate_ce_loss(self, y, y_len, x=None, image_features=None, image_feature_map=None, **kwargs):
        if image_feature_map is not None:
            raise NotImplementedError("attention language models are outside the implemented path")
        feats = (x if image_features is None else image_features) if self.text_encoder.captioning else None
        return self.language_model.calculate_ce_loss(y, y_len, image_features=feats, **kwargs)


def lm_args(captioning=False, **kw):
    base = dict(embedding_type="flat", embedding_dim=E, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False,
                vit_dino=False, finetune_cnn=False, text_encoder="lstm", captioning=captioning, attention=False, attention_gate=False,
                crange=1, dropout_i=0.0, dropout_o=0.0, pos_embed_type="no_pos_embed", normalize_features=False, sim="max",
                temperature=0.07, fix_temperature=False, tie=True, bias=True)
    base.update(kw)
    return argparse.Namespace(**base)


def toy_model(dev, captioning, **kw):
    from multimodal.multimodal import LanguageModel, TextEncoder
    args = lm_args(captioning, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(small_vocab(V), 2048, args)
        lm = LanguageModel(te, args)
    w = toy_weights(captioning)
    if args.text_encoder == "lstm":
        te.load_state_dict({k: v for k, v in w.items() if k != "out_bias"})
        with torch.no_grad():
            lm.output_layer.bias.copy_(w["out_bias"])
    return StubLit(lm).to(dev).eval(), w


def restate(w, batches, pos_tags, captioning, dtype=torch.float64):
    """The reference's values from the weights, in ``dtype`` on the CPU -> (losses [n_utt, Lmax] zero-padded,
    token_pos {(token_id, pos): [cnt, loss, vector]} summed in visiting order, probs [(key, row [V])] with the leading zero row)."""
    w = {k: v.detach().cpu().to(dtype) for k, v in w.items()}
    lstm = torch.nn.LSTM(E, E, batch_first=True).to(dtype)
    with torch.no_grad():
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(lstm, k).copy_(w["lstm." + k])
    lmax = max(b[1].shape[1] for b in batches)
    losses, token_pos, probs = [], {}, []
    tags_it = iter(pos_tags)
    with torch.no_grad():
        for x, y, y_len, _raw in batches:
            B, L = y.shape
            state = None
            if captioning:
                st = x.to(dtype) @ w["connector.weight"].t() + w["connector.bias"]
                state = (st[:, :E].contiguous()[None], st[:, E:].contiguous()[None])
            out, _ = lstm(w["embedding.weight"][y], state)                    # unpacked: a position never sees what follows it
            logits = out[:, :-1] @ w["embedding.weight"].t() + w["out_bias"]
            loss = F.cross_entropy(logits.reshape(B * (L - 1), V), y[:, 1:].reshape(-1), ignore_index=0, reduction="none")
            loss = F.pad(loss.view(B, L - 1), (1, 0))
            p = F.pad(logits.softmax(-1), (0, 0, 1, 0))
            for b in range(B):
                n = int(y_len[b])
                row = torch.zeros(lmax, dtype=dtype)
                row[:n] = loss[b, :n]
                losses.append(row)
                for l, tag in enumerate(next(tags_it)[:n]):
                    key = (int(y[b, l]), tag)
                    item = token_pos.setdefault(key, [0, torch.zeros((), dtype=torch.float64), torch.zeros(E, dtype=dtype)])
                    item[0] += 1
                    item[1] = item[1] + loss[b, l].double()
                    item[2] = item[2] + out[b, l]
                    probs.append((key, p[b, l]))
    return torch.stack(losses), token_pos, probs


def merge_by_word(token_pos):
    """get_token_items on the restated table: {(token_id, majority pos): [cnt, loss, vector]}, majority = max over (cnt, pos)."""
    out = {}
    for tok in sorted({k[0] for k in token_pos}):
        group = sorted((k, v) for k, v in token_pos.items() if k[0] == tok)
        key = max(group, key=lambda kv: (kv[1][0], kv[0][1]))[0]
        out[key] = [sum(v[0] for _k, v in group), sum(v[1] for _k, v in group), sum(v[2] for _k, v in group)]
    return out


def stored_items(z, name, table):
    """The reference's table from the fixture -> (keys [(token_id, pos)], cnt, loss, vector) in sorted key order."""
    pre = f"{name}.{table}."
    keys = list(zip(z[pre + "token_id"].tolist(), z[pre + "pos"].tolist()))
    return keys, z[pre + "cnt"], z[pre + "loss"], z[pre + "vector"]


def topk_logits(R, Vn, k, seed):
    """Logits whose k + 1 best probabilities are well separated in every row: rank r of a random permutation gets -0.3 r plus a
    jitter of +-0.02 -- neighbouring probabilities differ by >= 23 % -- and one row in three is shifted by a large constant."""
    g = torch.Generator().manual_seed(seed)
    rank = torch.stack([torch.randperm(Vn, generator=g) for _ in range(R)]).float()
    lg = -0.3 * rank + (torch.rand(R, Vn, generator=g) - 0.5) * 0.04
    lg[::3] += 37.5
    labels = torch.randint(1, Vn, (R,), generator=g)
    labels[::4] = 0                                                          # <pad>
    return lg, labels


def topk_reference(logits, k):
    """float64: (top_prob [R, k], top_idx [R, k]) by (probability desc, index asc), the whole softmax, and the smallest gap among
    the k + 1 best probabilities of a row."""
    p = logits.double().softmax(-1)
    order = torch.from_numpy(np.lexsort((np.arange(p.shape[1])[None].repeat(p.shape[0], 0), -p.numpy()), axis=1))
    idx = order[:, :k]
    best = p.gather(1, order[:, :min(k + 1, p.shape[1])])
    gap = float((best[:, :-1] - best[:, 1:]).min()) if best.shape[1] > 1 else float("inf")
    return p.gather(1, idx), idx, p, gap
