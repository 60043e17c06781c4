"""Shared by the ViT self-attention tests: a plain torch restatement of the reference's VisionTransformer.get_last_selfattention and
get_intermediate_layers (vision_transformer_dino_mugs.py:252-269) over a ``state_dict`` (keys as the reference names them), in
whatever dtype the weights and the input come in -- float64 for the reference values, fp32 for the yardstick the bounds are derived
from, and under torch.autocast(bfloat16) for the bf16 yardstick.  tools/gen_golden_vit_attention.py checks it against the
reference's own class."""
import math

import torch
import torch.nn.functional as F


def _pos(pos_embed, gh, gw):
    """interpolate_pos_encoding (:210-230): the identity on the native square grid."""
    N = pos_embed.shape[1] - 1
    if gh * gw == N and gh == gw:
        return pos_embed
    D = pos_embed.shape[-1]
    s = int(math.sqrt(N))
    grid = pos_embed[:, 1:].reshape(1, s, s, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, scale_factor=((gh + 0.1) / math.sqrt(N), (gw + 0.1) / math.sqrt(N)), mode="bicubic")
    assert grid.shape[-2] == gh and grid.shape[-1] == gw
    return torch.cat([pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, D)], dim=1)


def depth_of(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def _walk(sd, x, patch, heads, eps):
    """Yields (i, tokens before block i, attention of block i, tokens after block i)."""
    dt = sd["cls_token"].dtype
    x = x.to(dt)
    B = x.shape[0]
    gh, gw = x.shape[2] // patch, x.shape[3] // patch
    D = sd["cls_token"].shape[-1]
    tok = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)   # :166
    h = torch.cat([sd["cls_token"].expand(B, -1, -1).to(tok.dtype), tok], dim=1) + _pos(sd["pos_embed"], gh, gw)              # :237-241
    T, hd = h.shape[1], D // heads
    for i in range(depth_of(sd)):
        p = f"blocks.{i}."
        y = F.layer_norm(h, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd.get(p + "attn.qkv.bias")).reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)                                                       # :123-124
        before = h
        o = (attn @ v).transpose(1, 2).reshape(B, T, D)
        h = h + F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])                                             # :147
        y = F.layer_norm(h, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        h = h + F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"],
                         sd[p + "mlp.fc2.bias"])                                                                              # :148
        yield i, before, attn, h


def last_selfattention(sd, x, patch, heads, eps=1e-6):
    """[B, heads, T, T]: the last block's softmax(q k^T scale)."""
    for i, _, attn, _ in _walk(sd, x, patch, heads, eps):
        pass
    return attn


def intermediate_layers(sd, x, patch, heads, n=1, eps=1e-6):
    """n tensors [B, T, D]: norm(tokens after block i) for the last n blocks, in block order."""
    depth, D = depth_of(sd), sd["cls_token"].shape[-1]
    return [F.layer_norm(h, (D,), sd["norm.weight"], sd["norm.bias"], eps)
            for i, _, _, h in _walk(sd, x, patch, heads, eps) if depth - i <= n]


def maps_and_layers(sd, x, patch, heads, n=1, eps=1e-6):
    """(last_selfattention, intermediate_layers) from one walk over the blocks."""
    depth, D = depth_of(sd), sd["cls_token"].shape[-1]
    layers = []
    for i, _, attn, h in _walk(sd, x, patch, heads, eps):
        if depth - i <= n:
            layers.append(F.layer_norm(h, (D,), sd["norm.weight"], sd["norm.bias"], eps))
    return attn, layers


def to_dtype(sd, dt):
    return {k: v.to(dt) for k, v in sd.items()}


def softmax_probs(qkv, B, T, heads, hd, scale, q_rows=None):
    """qkv [B T, 3 heads hd] in the dtype it comes in -> (q k^T * scale).softmax(-1)[:, :, :q_rows], [B, heads, q_rows, T]."""
    q, k, _ = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q = q[:, :, :q_rows] if q_rows is not None else q
    return ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)


def tau(ref32, ref64, factor=4.0):
    """The bound of the kernel tests: ``factor`` x the worst absolute error of torch's own fp32 CPU evaluation against float64 on the
    same inputs (the rule of tests/test_neighbors_gpu.py; 4 covers a different but equally valid summation order)."""
    return factor * float((ref32.double() - ref64).abs().max())
