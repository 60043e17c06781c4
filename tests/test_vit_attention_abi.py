"""CPU: the ViT self-attention entries (cvcl_attention_probs, cvcl_cls_attention_maps) are declared, bound and exported and refuse
invalid arguments with CVCL_EINVAL on dummy pointers without touching a GPU; VisionTransformer carries the reference's two analysis
methods with the reference's signatures; the Python layer refuses a ResNeXt encoder, CPU tensors and an ``n`` outside the depth."""
import argparse
import contextlib
import inspect
import io
import os
import re
from functools import partial

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_attention_probs", "cvcl_cls_attention_maps")
FAKE = 0x10000                                          # 16-byte aligned, never dereferenced: validation fails first
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    _hip.load()
    return _hip


def test_entries_declared_bound_exported(lib):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    l = lib.lib()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt) and l.cvcl_abi_version() == lib.ABI_VERSION == 7      # additive change
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", txt), name
        assert name in lib.SIGNATURES, name
        assert hasattr(l, name), name
    assert "vision_transformer_dino_mugs.py:252-259" in txt          # the reference lines the kernel serves
    assert os.path.exists(os.path.join(ROOT, "multimodal-baby_amd", "csrc", "vit_maps.hip"))


def _probs(lib, dtype=0, qkv=FAKE, probs=FAKE + 4096, B=2, T=197, heads=12, hd=64, scale=0.125, q_rows=197):
    return lib.lib().cvcl_attention_probs(dtype, qkv, probs, B, T, heads, hd, scale, q_rows, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(qkv=None), b"null"),
    (dict(probs=None), b"null"),
    (dict(q_rows=0), b"q_rows 0 outside 1 .. T = 197"),
    (dict(q_rows=-3), b"q_rows -3 outside"),
    (dict(q_rows=198), b"q_rows 198 outside 1 .. T = 197"),
    (dict(dtype=2), b"dtype 2 is not accepted"),                   # CVCL_F32X3 is a trunk dtype
    (dict(dtype=7), b"dtype 7 is not accepted"),
    (dict(dtype=-1), b"dtype -1 is not accepted"),
    (dict(B=0), b"sizes must be positive"),
    (dict(T=0, q_rows=1), b"sizes must be positive"),
    (dict(heads=0), b"sizes must be positive"),
    (dict(hd=0), b"head_dim 0"),
    (dict(hd=18), b"head_dim 18"),
    (dict(hd=132), b"head_dim 132"),
    (dict(hd=-64), b"head_dim -64"),
    (dict(scale=float("nan")), b"scale must be finite"),
    (dict(scale=float("inf")), b"scale must be finite"),
    (dict(qkv=FAKE + 4), b"16-byte aligned"),                      # the MFMA route's operand loads
    (dict(B=1 << 20, T=1 << 12, heads=64, q_rows=1 << 12), b"too large"),
])
def test_attention_probs_refusals(lib, kw, msg):
    assert _probs(lib, **kw) == EINVAL
    err = lib.lib().cvcl_last_error()
    assert msg in err and b"cvcl_attention_probs" in err


def test_cls_maps_refusals(lib):
    l = lib.lib()
    for args, msg in (((None, FAKE, 2, 12, 197, 1), b"null"), ((FAKE, None, 2, 12, 197, 1), b"null"),
                      ((FAKE, FAKE, 2, 12, 197, 1), b"alias"), ((FAKE, FAKE + 64, 0, 12, 197, 1), b"T > 1"),
                      ((FAKE, FAKE + 64, 2, 0, 197, 0), b"T > 1"), ((FAKE, FAKE + 64, 2, 12, 1, 1), b"T > 1")):
        assert l.cvcl_cls_attention_maps(*args, None) == EINVAL
        assert msg in l.cvcl_last_error()


def _tiny_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return vits.VisionTransformer(img_size=[32], patch_size=8, embed_dim=32, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_vision_transformer_has_the_reference_methods(lib):
    from multimodal.vision_transformer_dino_mugs import VisionTransformer
    sig = inspect.signature(VisionTransformer.get_last_selfattention)
    assert list(sig.parameters) == ["self", "x"]
    sig = inspect.signature(VisionTransformer.get_intermediate_layers)
    assert list(sig.parameters) == ["self", "x", "n"] and sig.parameters["n"].default == 1
    m = _tiny_vit()
    x = torch.zeros(1, 3, 32, 32)
    for n in (0, 3, -1, True, 1.0):
        with pytest.raises(ValueError, match="outside 1 .. depth = 2"):
            m.get_intermediate_layers(x, n)
    with pytest.raises(lib.CvclError, match="no CPU fallback"):
        m.get_last_selfattention(x)
    with pytest.raises(lib.CvclError, match="no CPU fallback"):
        m.get_intermediate_layers(x, 2)


def test_vit_cls_attention_refusals(lib):
    from multimodal import attention_maps as A
    from multimodal.multimodal import MultiModalModel
    from multimodal.multimodal_lit import MultiModalLitModel
    from multimodal.resnext import ResNet
    with contextlib.redirect_stdout(io.StringIO()):
        resnet = ResNet.__new__(ResNet)
        torch.nn.Module.__init__(resnet)
    enc = torch.nn.Module()
    enc.model = resnet
    for target in (resnet, enc):
        with pytest.raises(NotImplementedError, match="gradCAM_pairs"):
            A.vit_cls_attention(target, torch.zeros(1, 3, 32, 32))
    m = _tiny_vit()
    with pytest.raises(lib.CvclError, match="no CPU fallback"):
        A.vit_cls_attention(m, torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="heads"):
        A.vit_cls_attention(m, torch.zeros(1, 3, 32, 32), heads="max")
    assert callable(MultiModalModel.self_attention_maps) and callable(MultiModalLitModel.self_attention_maps)
    assert list(inspect.signature(MultiModalModel.self_attention_maps).parameters) == ["self", "image", "text", "text_length"]


def test_eval_help_names_the_vit_maps(lib):
    import eval as ev
    text = " ".join(ev._parser().format_help().split())
    assert "self-attention" in text and "do not depend on the label" in text
