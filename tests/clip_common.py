"""What the CLIP tests share: a float64 torch restatement of OpenAI's CLIP forward (ViT image tower, causal text tower, logits),
the OpenAI <-> ``transformers`` parameter-name mapping, a random state dict in OpenAI layout, and a synthetic BPE merges file learned
from the words of multimodal/vocab.json.  Nothing here touches the GPU or the package under test."""
import collections
import json
import os

import torch
import torch.nn.functional as F

from conftest import ROOT

IGNORED = ("input_resolution", "context_length", "vocab_size")


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


def _ident(t):
    return t


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _ln(x, sd, name):
    return F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], 1e-5)


def _lin(x, w, b, rnd):
    y = rnd(x) @ rnd(w).t()
    return y if b is None else y + b


def _resblocks(x, sd, prefix, causal, rnd):
    """x [B, T, W]; pre-LN blocks, heads of 64, scale 64^-0.5, QuickGELU; ``rnd`` rounds the operands of every linear."""
    n = len({k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)})
    B, T, W = x.shape
    heads = W // 64
    for i in range(n):
        p = f"{prefix}{i}."
        y = _lin(_ln(x, sd, p + "ln_1"), sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"], rnd)
        q, k, v = (rnd(y).reshape(B, T, 3, heads, 64)[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(-1, -2) * 64 ** -0.5
        if causal:
            s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
        a = (rnd(torch.softmax(s, -1)) @ v).permute(0, 2, 1, 3).reshape(B, T, W)
        x = rnd(x + rnd(_lin(a, sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"], rnd)))
        h = _lin(_ln(x, sd, p + "ln_2"), sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"], rnd)
        h = rnd(h * torch.sigmoid(1.702 * h))
        x = rnd(x + rnd(_lin(h, sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"], rnd)))
    return x


def encode_image(sd, image, rnd=_ident):
    """``rnd`` = bf16_round: the storage points of the bf16 image tower (linear operands, block outputs) rounded, float64 otherwise."""
    sd = {k: v.double() for k, v in sd.items() if k not in IGNORED}
    w = sd["visual.conv1.weight"]
    W, p = w.shape[0], w.shape[-1]
    B = image.shape[0]
    cols = F.unfold(image.double(), p, stride=p).transpose(1, 2)                      # [B, np, 3 p p]
    tok = _lin(cols, w.reshape(W, -1), None, rnd)
    cls = (sd["visual.class_embedding"] + sd["visual.positional_embedding"][0]).expand(B, 1, W)
    h = rnd(torch.cat([cls, rnd(tok) + sd["visual.positional_embedding"][1:]], 1))
    h = rnd(_ln(h, sd, "visual.ln_pre"))
    h = _resblocks(h, sd, "visual.transformer.resblocks.", False, rnd)
    return _ln(h[:, 0], sd, "visual.ln_post") @ sd["visual.proj"]


def encode_text(sd, tok):
    sd = {k: v.double() for k, v in sd.items() if k not in IGNORED}
    x = sd["token_embedding.weight"][tok] + sd["positional_embedding"]
    x = _resblocks(x, sd, "transformer.resblocks.", True, _ident)
    x = _ln(x, sd, "ln_final")
    return x[torch.arange(x.shape[0]), tok.argmax(-1)] @ sd["text_projection"]


def logits(sd, image, tok):
    i, t = encode_image(sd, image), encode_text(sd, tok)
    i, t = i / i.norm(dim=-1, keepdim=True), t / t.norm(dim=-1, keepdim=True)
    lpi = sd["logit_scale"].double().exp() * i @ t.t()
    return lpi, lpi.t()


# ---- state dicts ----------------------------------------------------------------------------------------------------------------
def random_state_dict(seed=0, W=128, layers=2, patch=14, R=84, Wt=128, tlayers=2, vocab=512, ctx=77, E=64, scale=2.0):
    """OpenAI layout, normal(0, 0.05) weights, LayerNorm weights 1 + noise."""
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g) * 0.05
    sd = {"visual.conv1.weight": rn(W, 3, patch, patch), "visual.class_embedding": rn(W),
          "visual.positional_embedding": rn((R // patch) ** 2 + 1, W), "visual.proj": rn(W, E),
          "token_embedding.weight": rn(vocab, Wt), "positional_embedding": rn(ctx, Wt), "text_projection": rn(Wt, E),
          "logit_scale": torch.tensor(float(scale))}

    def ln(name, w):
        sd[name + ".weight"], sd[name + ".bias"] = 1 + rn(w), rn(w)
    for name, w in (("visual.ln_pre", W), ("visual.ln_post", W), ("ln_final", Wt)):
        ln(name, w)
    for prefix, w, n in (("visual.transformer.resblocks.", W, layers), ("transformer.resblocks.", Wt, tlayers)):
        for i in range(n):
            p = f"{prefix}{i}."
            ln(p + "ln_1", w)
            ln(p + "ln_2", w)
            sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = rn(3 * w, w), rn(3 * w)
            sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(w, w), rn(w)
            sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = rn(4 * w, w), rn(4 * w)
            sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = rn(w, 4 * w), rn(w)
    return sd


def from_transformers(hf):
    """``transformers.CLIPModel`` state dict -> OpenAI names."""
    out = {"logit_scale": hf["logit_scale"], "visual.proj": hf["visual_projection.weight"].t(),
           "text_projection": hf["text_projection.weight"].t(),
           "visual.conv1.weight": hf["vision_model.embeddings.patch_embedding.weight"],
           "visual.class_embedding": hf["vision_model.embeddings.class_embedding"],
           "visual.positional_embedding": hf["vision_model.embeddings.position_embedding.weight"],
           "token_embedding.weight": hf["text_model.embeddings.token_embedding.weight"],
           "positional_embedding": hf["text_model.embeddings.position_embedding.weight"]}
    for ours, theirs in (("visual.ln_pre", "vision_model.pre_layrnorm"), ("visual.ln_post", "vision_model.post_layernorm"),
                         ("ln_final", "text_model.final_layer_norm")):
        for k in ("weight", "bias"):
            out[f"{ours}.{k}"] = hf[f"{theirs}.{k}"]
    for ours, theirs in (("visual.transformer.resblocks.", "vision_model.encoder.layers."), ("transformer.resblocks.", "text_model.encoder.layers.")):
        for i in sorted({int(k[len(theirs):].split(".")[0]) for k in hf if k.startswith(theirs)}):
            o, t = f"{ours}{i}.", f"{theirs}{i}."
            for k in ("weight", "bias"):
                out[o + "attn.in_proj_" + k] = torch.cat([hf[f"{t}self_attn.{n}_proj.{k}"] for n in "qkv"], 0)
                out[o + "attn.out_proj." + k] = hf[t + "self_attn.out_proj." + k]
                out[o + "ln_1." + k], out[o + "ln_2." + k] = hf[t + "layer_norm1." + k], hf[t + "layer_norm2." + k]
                out[o + "mlp.c_fc." + k], out[o + "mlp.c_proj." + k] = hf[t + "mlp.fc1." + k], hf[t + "mlp.fc2." + k]
    return {k: v.detach().clone() for k, v in out.items()}


# ---- a synthetic merges file ----------------------------------------------------------------------------------------------------
def vocab_words():
    with open(os.path.join(ROOT, "multimodal-baby_amd", "multimodal", "vocab.json")) as f:
        return list(json.load(f))


def learn_merges(words, n_merges=300):
    """Greedy BPE over ``words`` (each once, ``</w>`` on the last symbol), ties by the pair's text: a plausible, deterministic file."""
    seqs = [tuple(w[:-1]) + (w[-1] + "</w>",) for w in words if w and all(33 <= ord(c) < 127 for c in w)]
    merges = []
    for _ in range(n_merges):
        cnt = collections.Counter()
        for s in seqs:
            cnt.update(zip(s[:-1], s[1:]))
        if not cnt:
            break
        best = min(cnt, key=lambda p: (-cnt[p], p))
        merges.append(best)
        new = []
        for s in seqs:
            o, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and (s[i], s[i + 1]) == best:
                    o.append(s[i] + s[i + 1])
                    i += 2
                else:
                    o.append(s[i])
                    i += 1
            new.append(tuple(o))
        seqs = new
    return merges


def write_merges(path, merges):
    with open(path, "w", encoding="utf-8") as f:
        f.write("#version: synthetic\n" + "".join(f"{a} {b}\n" for a, b in merges))
    return str(path)
