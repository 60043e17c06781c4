"""CPU: the 32-split precision's host surface -- ABI v7 and CVCL_F32X3 in the header, the binding and the library; the
Trainer --precision mapping (with "32" and "bf16" mapped exactly as before); eval.py --precision."""
import os
import re
import types

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    return _hip


def _header():
    with open(os.path.join(ROOT, "include", "cvcl_hip.h")) as f:
        return f.read()


def test_abi_v7_and_f32x3_declared(H):
    hdr = _header()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", hdr)
    assert re.search(r"CVCL_F32X3 = 2\b", hdr)
    assert "CVCL_F32X3" in hdr.split("#ifndef CVCL_HIP_H")[0]          # documented in the Conventions block
    assert H.ABI_VERSION == 7 and H.F32X3 == 2 and (H.F32, H.BF16) == (0, 1)
    assert H.load().cvcl_abi_version() == 7


def test_size_queries_without_gpu(H):
    lib = H.load()
    # three bf16 parts per element: dense [3][cout][cin]; stem / grouped 3x3 [3][cout / 32][steps][32][16] (10 / 18 steps of 16 k)
    assert lib.cvcl_packed_weight_bytes(H.F32X3, H.PACK_DENSE, 256, 64, 1) == 256 * 64 * 3 * 2
    assert lib.cvcl_packed_weight_bytes(H.F32X3, H.PACK_GCONV3, 128, 4, 3) == 3 * 4 * 18 * 512 * 2
    assert lib.cvcl_packed_weight_bytes(H.F32X3, H.PACK_STEM7, 64, 3, 7) == 3 * 2 * 10 * 512 * 2
    assert lib.cvcl_resnext50_workspace_bytes(H.F32X3, 2, 64, 64) == lib.cvcl_resnext50_workspace_bytes(H.F32, 2, 64, 64)
    for bad in (3, -1, 99):
        assert lib.cvcl_packed_weight_bytes(bad, H.PACK_DENSE, 256, 64, 1) == 0
        assert lib.cvcl_resnext50_workspace_bytes(bad, 2, 64, 64) == 0
    # unknown dtypes are refused before any pointer is looked at
    for bad in (3, -1):
        assert lib.cvcl_pack_conv_weight(bad, H.PACK_DENSE, None, None, 1, 1, 1, None) == -1
        assert b"dtype" in lib.cvcl_last_error()
    for dt in (2, 3):
        assert lib.cvcl_layernorm(dt, None, 64, None, None, 1e-5, None, 1, 16, 64, None) == -1
        assert b"dtype" in lib.cvcl_last_error()


def _lit_stub(vit=False, finetune=False):
    from multimodal.multimodal_lit import MultiModalLitModel
    calls = []
    model = types.SimpleNamespace(fp8_linears=None)
    ve = types.SimpleNamespace(vit_dino=vit, model=model,
                               set_compute_dtype=lambda dt, arith="exact": calls.append((dt, arith)))
    te = types.SimpleNamespace()
    lit = types.SimpleNamespace(vision_encoder=ve, text_encoder=te)
    return lit, calls, MultiModalLitModel.set_precision


@pytest.mark.parametrize("p,dt,arith,split", [
    ("32", torch.float32, "exact", False), ("bf16", torch.bfloat16, "exact", True), ("16", torch.bfloat16, "exact", True),
    ("bf16-mixed", torch.bfloat16, "exact", True), ("fp8", torch.bfloat16, "exact", True), ("32-split", torch.float32, "split", True),
    (32, torch.float32, "exact", False)])
def test_set_precision_mapping(H, p, dt, arith, split):
    lit, calls, set_precision = _lit_stub()
    set_precision(lit, p)
    assert calls == [(dt, arith)]
    assert lit.text_encoder.__dict__["fp32_split"] is split


def test_set_compute_dtype_refusals(H):
    from multimodal.multimodal import VisionEncoder
    enc = VisionEncoder.__new__(VisionEncoder)
    torch.nn.Module.__init__(enc)
    enc.model = types.SimpleNamespace(compute_dtype=torch.float32, trunk_arithmetic="exact")
    enc.vit_dino, enc.finetune_cnn = False, False
    enc.set_compute_dtype(torch.float32, "split")
    assert enc.model.trunk_arithmetic == "split"
    enc.set_compute_dtype(torch.float32)
    assert enc.model.trunk_arithmetic == "exact"
    with pytest.raises(H.CvclError, match="32-split"):
        enc.set_compute_dtype(torch.bfloat16, "split")
    for attr in ("vit_dino", "finetune_cnn"):
        setattr(enc, attr, True)
        with pytest.raises(H.CvclError, match="32-split"):
            enc.set_compute_dtype(torch.float32, "split")
        assert enc.model.trunk_arithmetic == "exact"
        setattr(enc, attr, False)


def test_resnet_trunk_dtype(H):
    from multimodal.resnext import ResNet
    m = ResNet()
    assert m.trunk_arithmetic == "exact" and m.trunk_dtype() == H.F32
    m.trunk_arithmetic = "split"
    assert m.trunk_dtype() == H.F32X3
    m.compute_dtype = torch.bfloat16                 # bf16 storage has no split form: the arithmetic applies to fp32 only
    assert m.trunk_dtype() == H.BF16


def test_eval_precision_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_eval_cli", os.path.join(ROOT, "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    assert ev._parser().parse_args([]).precision == "32"
    for p in ("32", "bf16", "32-split"):
        assert ev._parser().parse_args(["--precision", p]).precision == p
    with pytest.raises(SystemExit):
        ev._parser().parse_args(["--precision", "fp16"])
