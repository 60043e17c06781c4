"""CPU: the discard entry of the attention rollout (cvcl_attention_discard) is declared, bound and exported, refuses invalid arguments
with CVCL_EINVAL on dummy pointers without touching a GPU, and returns CVCL_OK for k = 0 without a launch; the Python layers refuse
a discard_ratio outside 0 <= r < 1 (or one that is no number) and a k outside 0 .. T*T - 1 with ValueError before any launch;
eval.py has --rollout_discard_ratio and refuses it without --attention_rollout."""
import inspect
import os
import re
from functools import partial

import pytest
import torch

from conftest import ROOT

FAKE = 0x10000                                          # never dereferenced: validation fails first, k = 0 launches nothing
OK, EINVAL = 0, -1
BAD_RATIOS = (-0.1, 1.0, 1.5, True, "0.9", float("nan"))


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


def test_entry_declared_bound_exported(lib):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    l = lib.lib()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt) and l.cvcl_abi_version() == lib.ABI_VERSION == 7      # additive change
    assert re.search(r"\bint cvcl_attention_discard\s*\(float\* fused, int n_mats, int T, long k, void\* stream\)", txt)
    assert "cvcl_attention_discard" in lib.SIGNATURES and hasattr(l, "cvcl_attention_discard")
    assert os.path.exists(os.path.join(ROOT, "multimodal-baby_amd", "csrc", "vit_discard.hip"))


def _discard(lib, fused=FAKE, n_mats=24, T=197, k=34928):
    return lib.lib().cvcl_attention_discard(fused, n_mats, T, k, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(fused=None), b"null"),
    (dict(n_mats=0), b"n_mats 0"),
    (dict(n_mats=-3), b"n_mats -3"),
    (dict(T=0, k=0), b"T 0 outside 1 .. 4096"),
    (dict(T=-5, k=0), b"T -5 outside 1 .. 4096"),
    (dict(T=4097, k=1), b"T 4097 outside 1 .. 4096"),
    (dict(k=-1), b"k -1 outside 0 .. T*T - 1 = 38808"),
    (dict(k=38809), b"k 38809 outside 0 .. T*T - 1 = 38808"),
    (dict(T=1, k=1), b"k 1 outside 0 .. T*T - 1 = 0"),
    (dict(T=4096, k=1 << 24), b"k 16777216 outside 0 .. T*T - 1 = 16777215"),
    (dict(k=1 << 40), b"k 1099511627776 outside"),                 # k travels as a 64-bit integer
])
def test_discard_refusals(lib, kw, msg):
    assert _discard(lib, **kw) == EINVAL
    err = lib.lib().cvcl_last_error()
    assert msg in err and b"cvcl_attention_discard" in err


@pytest.mark.parametrize("T", [1, 17, 197, 4096])
def test_k_zero_is_ok_without_a_device(lib, T):
    assert _discard(lib, T=T, k=0) == OK                   # the pointer is a dummy: a launch would fault, a device call would fail here
    assert _discard(lib, fused=None, T=T, k=0) == EINVAL   # (the argument checks still come first)


def _tiny_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return vits.VisionTransformer(img_size=[32], patch_size=8, embed_dim=32, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_discard_ratio_refused_before_any_launch(lib):
    """CPU tensors throughout: every ValueError comes before the device check, which then refuses the valid call."""
    from multimodal import attention_maps as A
    from multimodal import vit_maps
    sig = inspect.signature(vit_maps.attention_rollout)
    assert list(sig.parameters)[-1] == "discard_ratio" and sig.parameters["discard_ratio"].default == 0.0      # trailing, off
    assert list(inspect.signature(A.vit_attention_rollout_discard).parameters) == ["vision_model", "x", "discard_ratio", "size",
                                                                                  "head_fusion", "start_layer"]
    m = _tiny_vit()
    x = torch.zeros(1, 3, 32, 32)                           # T = 17, depth 2
    for r in BAD_RATIOS:
        with pytest.raises(ValueError, match="discard_ratio"):
            vit_maps.attention_rollout(m, x, discard_ratio=r)
        with pytest.raises(ValueError, match="discard_ratio"):
            vit_maps.attention_rollout(m, x, "max", 1, 17, None, r)
        with pytest.raises(ValueError, match="discard_ratio"):
            A.vit_attention_rollout_discard(m, x, r)
        with pytest.raises(ValueError, match="discard_ratio"):
            vit_maps.check_discard_ratio(r)
    for r in (0, 0.0, 0.5, 0.9, 0.999):
        assert vit_maps.check_discard_ratio(r) == float(r)
        with pytest.raises(lib.CvclError, match="no CPU fallback"):
            vit_maps.attention_rollout(m, x, discard_ratio=r)
        with pytest.raises(lib.CvclError, match="no CPU fallback"):
            A.vit_attention_rollout_discard(m, x, r)
    with pytest.raises(ValueError, match="head_fusion"):    # the other refusals stand next to the new one
        A.vit_attention_rollout_discard(m, x, 0.9, head_fusion="median")
    with pytest.raises(ValueError, match="start_layer"):
        A.vit_attention_rollout_discard(m, x, 0.9, start_layer=2)


def test_attention_discard_host_refusals(lib):
    from multimodal import vit_maps
    slab = torch.zeros(2, 1, 17, 17)
    for k in (-1, 289, 1 << 40, 1.0, True, None):
        with pytest.raises(ValueError, match="k = "):
            vit_maps.attention_discard(slab, k)
    for bad in (torch.zeros(2, 17, 17), torch.zeros(2, 1, 17, 16), torch.zeros(2, 1, 17, 17, dtype=torch.float64),
                torch.zeros(2, 1, 17, 34)[..., ::2]):
        with pytest.raises(lib.CvclError, match="contiguous fp32"):
            vit_maps.attention_discard(bad, 1)
    with pytest.raises(lib.CvclError):                      # a CPU tensor has no device pointer
        vit_maps.attention_discard(slab, 1)


def test_eval_has_the_discard_flag(lib):
    import eval as ev
    assert ev._parser().parse_args(["--checkpoint", "c"]).rollout_discard_ratio == 0.0
    args = ev._parser().parse_args(["--checkpoint", "c", "--attention_rollout", "--rollout_discard_ratio", "0.9"])
    assert args.rollout_discard_ratio == 0.9 and args.attention_rollout is True
    text = " ".join(ev._parser().format_help().split())
    assert "--rollout_discard_ratio R" in text and "--attention_rollout" in text
    base = ["--checkpoint", "c", "--eval_dataset", "synthetic", "--attention_maps", "d"]
    with pytest.raises(SystemExit, match="--attention_rollout"):            # before anything is loaded
        ev.main(ev._parser().parse_args(base + ["--rollout_discard_ratio", "0.9"]))
    for r in ("-0.1", "1.0", "1.5", "nan"):
        with pytest.raises(SystemExit, match="--rollout_discard_ratio"):
            ev.main(ev._parser().parse_args(base + ["--attention_rollout", "--rollout_discard_ratio", r]))
    assert "discard_ratio" in inspect.signature(ev.evaluate_trials).parameters
