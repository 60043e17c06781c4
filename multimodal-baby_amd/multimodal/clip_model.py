"""OpenAI-layout CLIP (ViT image tower + causal text transformer) on libcvcl_hip: the model behind ``eval.py --clip_eval``
(reference eval.py:29-45, 205-207, 224-226, which calls the ``clip`` package's ``load`` / ``tokenize`` / ``model(image, text)``).

The module tree carries OpenAI's parameter names, so a released ``state_dict`` loads as it is; no ``forward`` of a submodule is a
torch composition -- the towers are walks over HIP kernels, and CPU tensors raise ``CvclError`` (no fallback, as everywhere here).

Image tower: ``vit_hip._Trunk`` (the DINO ViT's walk) over this model's packed-weight dict: no patch bias, ``ln_pre`` on the assembled
tokens, QuickGELU in the MLP, ``ln_post`` of the CLS rows and the ``visual.proj`` GEMM.  fp32 or bf16 (``set_precision``).
Text tower: always fp32 -- cvcl_embed_gather_pos, per block cvcl_layernorm / fp32 GEMMs / cvcl_attention_causal / QuickGELU epilogue,
then cvcl_clip_text_pool (end-of-text row + ``ln_final``) and the ``text_projection`` GEMM.  Logits: ops.l2_normalize + ops.sim_logits.

Weights and the BPE merges file are the user's: nothing is shipped or fetched.  ``tokenize`` restates ``clip.tokenize`` without ftfy's
Unicode repair."""
from __future__ import annotations

import gzip
import math
import unicodedata
from collections import OrderedDict
from functools import lru_cache

import torch
from torch import nn

from . import _hip as H
from . import ops
from .multimodal_data_module import CLIP_MEAN, CLIP_STD      # the frame statistics of CLIP's transform (noqa: F401, re-exported)
from .trunk_runtime import TrunkRuntime, fingerprint, strip
from .vit_hip import _Trunk, _ln

MAX_TOKENS = 288                       # cvcl_attention's bf16 MFMA kernel (ViT-L/14 at 224: 257; ViT-L/14@336 has 577: refused)
_IGNORED_KEYS = ("input_resolution", "context_length", "vocab_size")
_F = torch.float32


def _f(p):
    return p.detach().float().contiguous()


def _getstate(self):
    return strip(self.__dict__, "runtime")            # (__dict__: the instance's own state is what pickles; the runtime never is)


def _setstate(self, d):
    nn.Module.__setstate__(self, strip(d, "runtime"))     # (a pickle of an earlier version: its ``_cache`` is dropped)
    self.runtime = TrunkRuntime()


class _Held(nn.Module):
    """A module that only holds parameters under OpenAI's names: the arithmetic is in the HIP walks of CLIP."""

    def forward(self, *a, **k):
        raise H.CvclError(f"{type(self).__name__} holds parameters only: run the model through CLIP.encode_image / encode_text")


class _Attention(_Held):
    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * width))
        self.out_proj = nn.Linear(width, width)


class ResidualAttentionBlock(_Held):
    def __init__(self, width):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = _Attention(width)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, 4 * width)), ("c_proj", nn.Linear(4 * width, width))]))


class Transformer(_Held):
    def __init__(self, width, layers):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, width // 64
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width) for _ in range(layers)])

    def packed_blocks(self, dt):
        """The blocks in the key layout ``_Trunk.block`` reads; linears in ``dt``, LayerNorm parameters and biases fp32."""
        out = []
        for b in self.resblocks:
            out.append({
                "n1w": _f(b.ln_1.weight), "n1b": _f(b.ln_1.bias), "qkv_w": b.attn.in_proj_weight.detach().to(dt).contiguous(),
                "qkv_b": _f(b.attn.in_proj_bias), "proj_w": b.attn.out_proj.weight.detach().to(dt).contiguous(),
                "proj_b": _f(b.attn.out_proj.bias), "n2w": _f(b.ln_2.weight), "n2b": _f(b.ln_2.bias),
                "fc1_w": b.mlp.c_fc.weight.detach().to(dt).contiguous(), "fc1_b": _f(b.mlp.c_fc.bias),
                "fc2_w": b.mlp.c_proj.weight.detach().to(dt).contiguous(), "fc2_b": _f(b.mlp.c_proj.bias),
                "eps": b.ln_1.eps, "scale": 64 ** -0.5, "heads": self.heads})
        return out


class VisionTransformer(_Held):
    def __init__(self, input_resolution, patch_size, width, layers, output_dim):
        super().__init__()
        self.input_resolution, self.patch_size, self.embed_dim, self.output_dim = input_resolution, patch_size, width, output_dim
        self.conv1 = nn.Conv2d(3, width, patch_size, patch_size, bias=False)
        self.class_embedding = nn.Parameter(torch.empty(width))
        self.positional_embedding = nn.Parameter(torch.empty((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(torch.empty(width, output_dim))
        self.compute_dtype = torch.float32
        self.runtime = TrunkRuntime()

    __getstate__, __setstate__ = _getstate, _setstate

    def packed_weights(self, dt, device):
        """vit_hip._Trunk's packed-weight dict for this tower (cast once per weight version)."""
        return self.runtime.cache.get("w", fingerprint(self.parameters(), str(dt), str(device)), lambda: self._pack(dt, device))

    def _pack(self, dt, device):
        D, p = self.embed_dim, self.patch_size
        K = 3 * p * p
        Kpad = (K + 7) // 8 * 8
        wp = torch.zeros(D, Kpad, dtype=_F, device=device)
        wp[:, :K] = self.conv1.weight.detach().reshape(D, K)
        w = {"pe_w": wp.to(dt).contiguous(), "Kpad": Kpad, "pe_b": None, "cls": _f(self.class_embedding),
             "pos": _f(self.positional_embedding), "pre": (_f(self.ln_pre.weight), _f(self.ln_pre.bias), self.ln_pre.eps),
             "act": H.ACT_QUICK_GELU, "blocks": self.transformer.packed_blocks(dt),
             "nw": _f(self.ln_post.weight), "nb": _f(self.ln_post.bias), "neps": self.ln_post.eps,
             "proj": _f(self.proj.t())}                     # [E, D]: cvcl_gemm's W layout
        if torch.device(device).type == "cuda":
            torch.cuda.current_stream(device).synchronize()
        return w


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_layers):
        super().__init__()
        for name, width in (("vision", vision_width), ("text", transformer_width)):
            if width % 64 or width <= 0:
                raise H.CvclError(f"CLIP {name} width {width} is not a multiple of 64 (heads = width / 64, head_dim 64)")
        tokens = (image_resolution // vision_patch_size) ** 2 + 1
        if tokens > MAX_TOKENS:
            raise H.CvclError(f"CLIP image tower with {tokens} tokens (resolution {image_resolution}, patch {vision_patch_size}): the "
                              f"attention kernel takes T <= {MAX_TOKENS} (ViT-L/14@336 is out of scope)")
        self.context_length, self.vocab_size = context_length, vocab_size
        self.visual = VisionTransformer(image_resolution, vision_patch_size, vision_width, vision_layers, embed_dim)
        self.transformer = Transformer(transformer_width, transformer_layers)
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.runtime = TrunkRuntime()
        self.initialize_parameters()

    __getstate__, __setstate__ = _getstate, _setstate

    def initialize_parameters(self):
        """The ``clip`` package's random initialisation (model.py: initialize_parameters)."""
        with torch.no_grad():
            nn.init.normal_(self.token_embedding.weight, std=0.02)
            nn.init.normal_(self.positional_embedding, std=0.01)
            v = self.visual
            nn.init.normal_(v.conv1.weight, std=0.02)
            nn.init.normal_(v.class_embedding, std=v.embed_dim ** -0.5)
            nn.init.normal_(v.positional_embedding, std=v.embed_dim ** -0.5)
            nn.init.normal_(v.proj, std=v.embed_dim ** -0.5)
            for t in (self.transformer, v.transformer):
                proj_std = (t.width ** -0.5) * ((2 * t.layers) ** -0.5)
                for b in t.resblocks:
                    nn.init.normal_(b.attn.in_proj_weight, std=t.width ** -0.5)
                    nn.init.zeros_(b.attn.in_proj_bias)
                    nn.init.normal_(b.attn.out_proj.weight, std=proj_std)
                    nn.init.normal_(b.mlp.c_fc.weight, std=(2 * t.width) ** -0.5)
                    nn.init.normal_(b.mlp.c_proj.weight, std=proj_std)
            nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    @property
    def dtype(self):
        return self.visual.compute_dtype

    def set_precision(self, precision):
        """"32": fp32 storage and arithmetic; "bf16": the image tower's tokens and linears in bf16 (fp32 accumulation, statistics and
        projection).  The text tower is fp32 in both.  fp8 and 32-split exist for the DINO ViT / ResNeXt trunks only."""
        p = str(precision)
        if p not in ("32", "bf16"):
            raise H.CvclError(f"CLIP runs in precision '32' or 'bf16', not {precision!r} (32-split and fp8 are not built for it)")
        self.visual.compute_dtype = torch.float32 if p == "32" else torch.bfloat16
        return self

    # ---- towers ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_image(self, image):
        v = self.visual
        if not torch.is_tensor(image) or not image.is_cuda:
            raise H.CvclError("CLIP.encode_image needs device tensors (got a CPU tensor); there is no CPU fallback")
        if image.dim() != 4 or image.shape[2] != v.input_resolution or image.shape[3] != v.input_resolution:
            raise H.CvclError(f"CLIP.encode_image expects [B, 3, {v.input_resolution}, {v.input_resolution}] images, got "
                              f"{tuple(image.shape)} (the position table is not resampled)")
        t = _Trunk(v, image.float()).tokens()
        for bw in t.w["blocks"]:
            t.block(bw)
        return t.features()

    def _text_weights(self, device):
        mods = nn.ModuleList([self.transformer, self.token_embedding, self.ln_final])
        key = fingerprint([*mods.parameters(), self.positional_embedding, self.text_projection], str(device))
        return self.runtime.cache.get("t", key, lambda: {
            "table": _f(self.token_embedding.weight), "pos": _f(self.positional_embedding), "blocks": self.transformer.packed_blocks(_F),
            "nw": _f(self.ln_final.weight), "nb": _f(self.ln_final.bias), "neps": self.ln_final.eps, "proj": _f(self.text_projection.t())})

    @torch.no_grad()
    def encode_text(self, text):
        if not torch.is_tensor(text) or not text.is_cuda:
            raise H.CvclError("CLIP.encode_text needs device tensors (got a CPU tensor); there is no CPU fallback")
        if text.dim() != 2 or text.shape[1] != self.context_length or text.dtype not in (torch.int64, torch.int32):
            raise H.CvclError(f"CLIP.encode_text expects [B, {self.context_length}] integer tokens, got {tuple(text.shape)} {text.dtype}")
        tok = text.long().contiguous()
        w = self._text_weights(tok.device)
        B, L = tok.shape
        V, D = w["table"].shape
        lib, s, dev = H.lib(), H.stream_ptr(), tok.device
        x = torch.empty(B * L, D, dtype=_F, device=dev)
        H.check(lib.cvcl_embed_gather_pos(H.ptr(w["table"]), H.ptr(tok), H.ptr(w["pos"]), H.ptr(x), B, L, D, V, s), "cvcl_embed_gather_pos")
        y, att = torch.empty_like(x), torch.empty_like(x)
        qkv = torch.empty(B * L, 3 * D, dtype=_F, device=dev)
        mid = torch.empty(B * L, 4 * D, dtype=_F, device=dev)
        for bw in w["blocks"]:
            _ln(H.F32, x, D, bw["n1w"], bw["n1b"], bw["eps"], y, False, B * L, D)
            H.gemm(y, bw["qkv_w"], out=qkv, bias=bw["qkv_b"])
            H.check(lib.cvcl_attention_causal(H.F32, H.ptr(qkv), H.ptr(att), B, L, bw["heads"], D // bw["heads"], bw["scale"], s),
                    "cvcl_attention_causal")
            H.gemm(att, bw["proj_w"], out=x, bias=bw["proj_b"], residual=x)
            _ln(H.F32, x, D, bw["n2w"], bw["n2b"], bw["eps"], y, False, B * L, D)
            H.gemm(y, bw["fc1_w"], out=mid, bias=bw["fc1_b"], act=H.ACT_QUICK_GELU)
            H.gemm(mid, bw["fc2_w"], out=x, bias=bw["fc2_b"], residual=x)
        pooled = torch.empty(B, D, dtype=_F, device=dev)
        H.check(lib.cvcl_clip_text_pool(H.ptr(x), H.ptr(tok), H.ptr(w["nw"]), H.ptr(w["nb"]), w["neps"], H.ptr(pooled), B, L, D, s),
                "cvcl_clip_text_pool")
        return H.gemm(pooled, w["proj"])

    @torch.no_grad()
    def forward(self, image, text):
        """-> (logits_per_image [Bi, Bt], logits_per_text [Bt, Bi]) = exp(logit_scale) * cosine similarities."""
        img = ops.l2_normalize(self.encode_image(image))
        txt = ops.l2_normalize(self.encode_text(text))
        logits = ops.sim_logits(img, txt, self.logit_scale.detach().float())
        return logits, logits.t()


# ---- state dicts ----------------------------------------------------------------------------------------------------------------
def build_model(state_dict):
    """A CLIP of the shapes the state dict implies (OpenAI ViT layout), weights loaded as fp32 (released files are fp16)."""
    sd = {k: v for k, v in state_dict.items() if k not in _IGNORED_KEYS}
    if "visual.proj" not in sd or "visual.conv1.weight" not in sd:
        raise H.CvclError("not an OpenAI ViT CLIP state dict (visual.conv1.weight / visual.proj missing; ResNet CLIPs are out of scope)")

    def layers(prefix):
        return len({k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)})
    vision_width, patch = sd["visual.conv1.weight"].shape[0], sd["visual.conv1.weight"].shape[-1]
    grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    model = CLIP(embed_dim=sd["text_projection"].shape[1], image_resolution=patch * grid, vision_layers=layers("visual.transformer.resblocks."),
                 vision_width=vision_width, vision_patch_size=patch, context_length=sd["positional_embedding"].shape[0],
                 vocab_size=sd["token_embedding.weight"].shape[0], transformer_width=sd["ln_final.weight"].shape[0],
                 transformer_layers=layers("transformer.resblocks."))
    model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return model.eval()


def normalize_frames(frames):
    """[.., 3, H, W] frames in [0, 1] -> CLIP's normalisation (the last step of the ``clip`` package's preprocess)."""
    mean = torch.tensor(CLIP_MEAN, dtype=frames.dtype, device=frames.device).view(3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=frames.dtype, device=frames.device).view(3, 1, 1)
    return (frames - mean) / std


def clip_preprocess(size=224, device=None):
    """CLIP's image transform (multimodal_data_module.py:259-266; the ``clip`` package's own) on the device: Resize(size, BICUBIC) ->
    CenterCrop(size) -> ToTensor -> Normalize(CLIP_MEAN, CLIP_STD) as a ``preprocess.DevicePreprocess``"""
    from .preprocess import DevicePreprocess
    return DevicePreprocess(size=size, mode="shorter_side_center_crop", mean=CLIP_MEAN, std=CLIP_STD, device=device)


def load(path, device="cuda"):
    """``clip.load`` for a local file: a TorchScript archive (OpenAI's released ``ViT-L-14.pt``) or a plain ``state_dict`` file
    (optionally under a ``state_dict`` key).  -> (model on ``device`` in eval mode, the frame normalisation)."""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
    return build_model(sd).to(device), normalize_frames


# ---- tokenizer ------------------------------------------------------------------------------------------------------------------
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")
_N_MERGES = 49152 - 256 - 2                      # the lines of bpe_simple_vocab_16e6.txt that clip's vocabulary uses


@lru_cache()
def bytes_to_unicode():
    """GPT-2's reversible byte -> printable unicode character table."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _kind(ch):
    if ch.isspace():
        return "s"
    c = unicodedata.category(ch)[0]
    return c if c in "LN" else "o"


def split_pieces(text):
    """CLIP's pattern ``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+`` as a scanner (the
    standard ``re`` module has no \\p classes): the alternatives in their order at each position, unmatched whitespace skipped."""
    out, i, n = [], 0, len(text)
    while i < n:
        hit = next((s for s in (SOT, EOT) + _CONTRACTIONS if text.startswith(s, i)), None)
        if hit is not None:
            out.append(hit)
            i += len(hit)
            continue
        k = _kind(text[i])
        j = i + 1
        if k in "Lo":
            while j < n and _kind(text[j]) == k:
                j += 1
        if k != "s":
            out.append(text[i:j])
        i = j
    return out


class SimpleTokenizer:
    def __init__(self, bpe_path):
        opener = gzip.open if str(bpe_path).endswith(".gz") else open
        with opener(bpe_path, "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")
        merges = [tuple(l.split()) for l in lines[1:_N_MERGES + 1]]            # line 0 is the header
        merges = [m for m in merges if len(m) == 2]
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + [SOT, EOT]
        self.encoder = {t: i for i, t in enumerate(vocab)}
        self.decoder = {i: t for t, i in self.encoder.items()}
        self.bpe_ranks = {m: i for i, m in enumerate(merges)}
        self.cache = {SOT: SOT, EOT: EOT}

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        self.cache[token] = " ".join(word)
        return self.cache[token]

    def encode(self, text):
        text = " ".join(text.split()).strip().lower()                     # whitespace_clean + lower (ftfy's repair: not built)
        ids = []
        for piece in split_pieces(text):
            token = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self.bpe(token).split(" "))
        return ids


@lru_cache(maxsize=4)
def _tokenizer(bpe_path):
    return SimpleTokenizer(bpe_path)


def tokenize(texts, bpe_path, context_length=77):
    """``clip.tokenize``: [n, context_length] int64 rows ``<|startoftext|> tokens <|endoftext|>`` padded with 0; a longer input raises."""
    if isinstance(texts, str):
        texts = [texts]
    tk = _tokenizer(str(bpe_path))
    sot, eot = tk.encoder[SOT], tk.encoder[EOT]
    out = torch.zeros(len(texts), context_length, dtype=torch.long)
    for i, text in enumerate(texts):
        ids = [sot] + tk.encode(text) + [eot]
        if len(ids) > context_length:
            raise RuntimeError(f"Input {text!r} is too long for context length {context_length}")
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.long)
    return out
