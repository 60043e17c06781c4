"""CPU: the grouped train-mode BatchNorm trunk entries (cvcl_resnext50_fwd_grouped and its workspace query) are declared,
bound and exported at ABI 7, and refuse bad arguments with CVCL_EINVAL without touching a GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

ENTRIES = ("cvcl_resnext50_fwd_grouped", "cvcl_resnext50_fwd_grouped_workspace_bytes")


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    _hip.load()
    return _hip


def test_entries_declared_bound_exported_at_abi_7(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt)
    lib = H.lib()
    assert lib.cvcl_abi_version() == 7 == H.ABI_VERSION
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name


def _call(H, dtype=0, B=8, Hh=64, W=64, group=4, ptrs=True, n_layers=53):
    lib = H.lib()
    fake = C.c_void_p(0x1000) if ptrs else None
    arr = (H.ConvBnParams * 53)()
    for p in arr:                                       # host-side table only: never dereferenced on the device here
        p.w = p.gamma = p.beta = 0x1000
    return lib.cvcl_resnext50_fwd_grouped(dtype, B, Hh, W, group, fake, arr, n_layers, fake, 1 << 40, fake, fake, 1e-5, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(group=0), b"group 0 < 1"),
    (dict(group=-2), b"group -2 < 1"),
    (dict(B=10, group=4), b"not a multiple of group"),
    (dict(B=0, group=1), b"not a multiple of group"),
    (dict(Hh=48), b"multiples of 32"),
    (dict(W=100), b"multiples of 32"),
    (dict(dtype=1), b"dtype 1 not supported"),
    (dict(dtype=3), b"dtype 3 not supported"),
    (dict(ptrs=False), b"null pointer"),
    (dict(n_layers=52), b"expected 53"),
])
def test_refusals_answer_einval_without_gpu(H, kw, msg):
    assert _call(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def test_null_layer_tensor_is_refused(H):
    lib = H.lib()
    arr = (H.ConvBnParams * 53)()
    for p in arr:
        p.w = p.gamma = p.beta = 0x1000
    arr[17].gamma = None
    fake = C.c_void_p(0x1000)
    assert lib.cvcl_resnext50_fwd_grouped(0, 8, 64, 64, 4, fake, arr, 53, fake, 1 << 40, fake, fake, 1e-5, None) == -1
    assert b"layer 17" in lib.cvcl_last_error()


def test_workspace_query(H):
    q = H.lib().cvcl_resnext50_fwd_grouped_workspace_bytes
    assert q(0, 256, 224, 224, 4) > 5 * 256 * 112 * 112 * 64 * 4
    assert q(2, 256, 224, 224, 4) == q(0, 256, 224, 224, 4)
    assert q(1, 256, 224, 224, 4) == 0                  # bf16: not built
    assert q(0, 10, 64, 64, 4) == 0 and q(0, 8, 64, 64, 0) == 0
    # a too-small workspace is refused before anything is enqueued
    lib = H.lib()
    arr = (H.ConvBnParams * 53)()
    for p in arr:
        p.w = p.gamma = p.beta = 0x1000
    fake = C.c_void_p(0x1000)
    assert lib.cvcl_resnext50_fwd_grouped(0, 8, 64, 64, 4, fake, arr, 53, fake, 16, fake, fake, 1e-5, None) == -3


def test_resnet_refuses_bad_groups_without_gpu(H):
    import torch
    from multimodal.resnext import ResNet
    m = ResNet().train()
    for prm in m.parameters():
        prm.requires_grad_(False)
    with pytest.raises(H.CvclError, match="divide"):
        m.trunk(torch.zeros(6, 3, 64, 64), bn_groups=4)
    m.compute_dtype = torch.bfloat16
    with pytest.raises(H.CvclError, match="bf16"):
        m.trunk(torch.zeros(8, 3, 64, 64), bn_groups=4)


def test_forward_without_groups_calls_trunk_as_before(H):
    """ResNet.forward's batch path calls trunk(x, defer_wait=True) exactly as it did, so a stand-in for ``trunk`` that knows
    nothing of bn_groups still works; inside grouped_bn(G) the groups reach trunk and are cleared afterwards."""
    import torch
    from multimodal.resnext import ResNet
    m = ResNet()
    m.fc = torch.nn.Identity()
    pooled, fmap = torch.ones(2, 2048), torch.zeros(2, 2048, 1, 1)
    m.trunk = lambda x, defer_wait=False: (pooled, fmap)
    assert m(torch.zeros(2, 3, 32, 32)) is pooled
    seen = []
    m.trunk = lambda x, defer_wait=False, bn_groups=None: seen.append(bn_groups) or (pooled, fmap)
    with m.grouped_bn(2):
        m(torch.zeros(2, 3, 32, 32))
    m(torch.zeros(2, 3, 32, 32))
    assert seen == [2, None]
