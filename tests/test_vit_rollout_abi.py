"""CPU: the attention-rollout entries (cvcl_attention_head_fuse, cvcl_attention_rollout) are declared, bound and exported and refuse
invalid arguments with CVCL_EINVAL on dummy pointers without touching a GPU; the Python layer refuses an unknown head fusion, a
start layer outside the depth and q_rows outside 1 .. T with ValueError before any launch, and a ResNeXt encoder with the message
of vit_cls_attention; self_attention_maps keeps its old call."""
import contextlib
import inspect
import io
import os
import re
from functools import partial

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_attention_head_fuse", "cvcl_attention_rollout")
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
    assert re.search(r"enum \{ CVCL_FUSE_MEAN = 0, CVCL_FUSE_MAX = 1, CVCL_FUSE_MIN = 2 \}", txt)
    assert (lib.FUSE_MEAN, lib.FUSE_MAX, lib.FUSE_MIN) == (0, 1, 2)
    assert os.path.exists(os.path.join(ROOT, "multimodal-baby_amd", "csrc", "vit_rollout.hip"))


def _fuse(lib, dtype=0, qkv=FAKE, fused=FAKE + 4096, B=2, T=197, heads=12, hd=64, scale=0.125, fuse=0):
    return lib.lib().cvcl_attention_head_fuse(dtype, qkv, fused, B, T, heads, hd, scale, fuse, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(qkv=None), b"null"),
    (dict(fused=None), b"null"),
    (dict(dtype=2), b"dtype 2 is not accepted"),                   # CVCL_F32X3 is a trunk dtype
    (dict(dtype=7), b"dtype 7 is not accepted"),
    (dict(dtype=-1), b"dtype -1 is not accepted"),
    (dict(B=0), b"sizes must be positive"),
    (dict(T=0), b"sizes must be positive"),
    (dict(heads=0), b"sizes must be positive"),
    (dict(hd=0), b"head_dim 0"),
    (dict(hd=18), b"head_dim 18"),
    (dict(hd=132), b"head_dim 132"),
    (dict(hd=-64), b"head_dim -64"),
    (dict(scale=float("nan")), b"scale must be finite"),
    (dict(scale=float("inf")), b"scale must be finite"),
    (dict(fuse=3), b"fuse 3"),
    (dict(fuse=-1), b"fuse -1"),
    (dict(qkv=FAKE + 4), b"16-byte aligned"),                      # the MFMA route's operand loads
])
def test_head_fuse_refusals(lib, kw, msg):
    assert _fuse(lib, **kw) == EINVAL
    err = lib.lib().cvcl_last_error()
    assert msg in err and b"cvcl_attention_head_fuse" in err


def _rollout(lib, fused=FAKE, out=FAKE + 4096, n_layers=12, B=2, T=197, start_layer=0, q_rows=1):
    return lib.lib().cvcl_attention_rollout(fused, out, n_layers, B, T, start_layer, q_rows, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(fused=None), b"null"),
    (dict(out=None), b"null"),
    (dict(out=FAKE), b"alias"),
    (dict(n_layers=0), b"n_layers 0 < 1"),
    (dict(n_layers=-2), b"n_layers -2 < 1"),
    (dict(B=0), b"sizes must be positive"),
    (dict(T=0), b"sizes must be positive"),
    (dict(T=961, q_rows=1), b"T 961 > 960"),
    (dict(start_layer=-1), b"start_layer -1 outside 0 .. n_layers - 1 = 11"),
    (dict(start_layer=12), b"start_layer 12 outside 0 .. n_layers - 1 = 11"),
    (dict(q_rows=0), b"q_rows 0 outside 1 .. T = 197"),
    (dict(q_rows=-3), b"q_rows -3 outside"),
    (dict(q_rows=198), b"q_rows 198 outside 1 .. T = 197"),
])
def test_rollout_refusals(lib, kw, msg):
    assert _rollout(lib, **kw) == EINVAL
    err = lib.lib().cvcl_last_error()
    assert msg in err and b"cvcl_attention_rollout" in err


def _tiny_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return vits.VisionTransformer(img_size=[32], patch_size=8, embed_dim=32, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_host_refusals_before_any_launch(lib):
    """CPU tensors throughout: every ValueError comes before the device check, which then refuses the valid call."""
    from multimodal import attention_maps as A
    from multimodal import vit_maps
    from multimodal.vision_transformer_dino_mugs import VisionTransformer
    sig = inspect.signature(VisionTransformer.get_attention_rollout)
    assert list(sig.parameters) == ["self", "x", "head_fusion", "start_layer", "q_rows"]
    assert [sig.parameters[k].default for k in ("head_fusion", "start_layer", "q_rows")] == ["mean", 0, 1]
    sig = inspect.signature(A.vit_attention_rollout)
    assert list(sig.parameters) == ["vision_model", "x", "size", "head_fusion", "start_layer"]
    m = _tiny_vit()
    x = torch.zeros(1, 3, 32, 32)                           # T = 17, depth 2
    for fusion in ("median", None, "MEAN"):
        with pytest.raises(ValueError, match="head_fusion"):
            m.get_attention_rollout(x, head_fusion=fusion)
        with pytest.raises(ValueError, match="head_fusion"):
            A.vit_attention_rollout(m, x, head_fusion=fusion)
    for s in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match="start_layer"):
            m.get_attention_rollout(x, start_layer=s)
        with pytest.raises(ValueError, match="start_layer"):
            A.vit_attention_rollout(m, x, start_layer=s)
    for q in (0, 18, -1, 1.0):
        with pytest.raises(ValueError, match="q_rows"):
            m.get_attention_rollout(x, q_rows=q)
    with pytest.raises(lib.CvclError, match="no CPU fallback"):
        m.get_attention_rollout(x, "max", 1, 17)
    with pytest.raises(lib.CvclError, match="no CPU fallback"):
        A.vit_attention_rollout(m, x)
    with pytest.raises(ValueError, match="head_fusion"):
        vit_maps.attention_head_fuse(torch.zeros(17, 96), 1, 17, 2, 16, 0.25, "sum")
    with pytest.raises(ValueError, match="start_layer"):
        vit_maps.rollout_chain(torch.zeros(2, 1, 17, 17), 2, 1)
    with pytest.raises(ValueError, match="q_rows"):
        vit_maps.rollout_chain(torch.zeros(2, 1, 17, 17), 0, 18)


def test_resnext_encoder_is_refused(lib):
    from multimodal import attention_maps as A
    from multimodal.resnext import ResNet
    with contextlib.redirect_stdout(io.StringIO()):
        resnet = ResNet.__new__(ResNet)
        torch.nn.Module.__init__(resnet)
    enc = torch.nn.Module()
    enc.model = resnet
    for target in (resnet, enc):
        with pytest.raises(NotImplementedError, match="gradCAM_pairs") as e:
            A.vit_attention_rollout(target, torch.zeros(1, 3, 32, 32))
        with pytest.raises(NotImplementedError) as e0:
            A.vit_cls_attention(target, torch.zeros(1, 3, 32, 32))
        assert str(e.value) == str(e0.value)


def test_self_attention_maps_keeps_its_old_call(lib):
    from multimodal.multimodal import MultiModalModel
    from multimodal.multimodal_lit import MultiModalLitModel
    assert list(inspect.signature(MultiModalModel.self_attention_maps).parameters) == ["self", "image", "text", "text_length"]
    sig = inspect.signature(MultiModalModel.attention_rollout_maps)
    assert list(sig.parameters) == ["self", "image", "text", "text_length", "head_fusion", "start_layer"]
    sig = inspect.signature(MultiModalLitModel.self_attention_maps)
    assert list(sig.parameters) == ["self", "x", "y", "y_len", "rollout", "head_fusion", "start_layer"]
    assert [sig.parameters[k].default for k in ("rollout", "head_fusion", "start_layer")] == [False, "mean", 0]
    assert all(sig.parameters[k].default is inspect.Parameter.empty for k in ("x", "y", "y_len"))


def test_eval_has_the_rollout_flag(lib):
    import eval as ev
    args = ev._parser().parse_args(["--checkpoint", "c"])
    assert args.attention_rollout is False
    assert ev._parser().parse_args(["--attention_rollout"]).attention_rollout is True
    text = " ".join(ev._parser().format_help().split())
    assert "attention rollout" in text and "ResNeXt" in text
