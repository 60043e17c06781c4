"""CPU: the fp32 ViT fine-tuning entries (csrc/vit_f32_train.hip) are exported and refuse what they do not support with
CVCL_EINVAL before anything is enqueued -- null pointers, head_dim != 64, T outside (32, 288], bad row shapes."""
import os

import pytest

from conftest import ROOT

EINVAL = -1


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    return _hip


def test_f32_finetune_entries_are_bound(H):
    names = ("cvcl_attention_train_f32", "cvcl_attention_bwd_f32", "cvcl_layernorm_bwd_rows_f32", "cvcl_gelu_f32",
             "cvcl_vit_tokens_bwd_f32", "cvcl_gemm_tn_colsum_f32", "cvcl_gemm_tn_colsum_f32_workspace_bytes")
    lib = H.load()
    for n in names:
        assert n in H.SIGNATURES and hasattr(lib, n), n
    assert lib.cvcl_abi_version() == 7


def test_attention_f32_refusals_without_gpu(H):
    lib = H.load()
    p = 4096                                                  # never dereferenced: every case is refused before a launch
    for hd, T in ((32, 197), (64, 32), (64, 289), (64, 0)):
        assert lib.cvcl_attention_train_f32(p, p, p, 2, T, 12, hd, 0.125, None) == EINVAL, (hd, T)
        assert lib.cvcl_attention_bwd_f32(p, p, p, p, p, 2, T, 12, hd, 0.125, None) == EINVAL, (hd, T)
    assert lib.cvcl_attention_train_f32(None, p, p, 2, 197, 12, 64, 0.125, None) == EINVAL
    assert lib.cvcl_attention_train_f32(p, p, None, 2, 197, 12, 64, 0.125, None) == EINVAL
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert lib.cvcl_attention_bwd_f32(*args, 2, 197, 12, 64, 0.125, None) == EINVAL, i
    assert b"cvcl_attention_bwd_f32" in lib.cvcl_last_error()


def test_other_f32_entries_refuse_bad_shapes(H):
    lib = H.load()
    p = 4096
    assert lib.cvcl_layernorm_bwd_rows_f32(p, 768, p, p, 768, 1e-6, None, p, 768, p, 10, 770, None) == EINVAL     # D % 4
    assert lib.cvcl_layernorm_bwd_rows_f32(p, 1028, p, p, 1028, 1e-6, None, p, 1028, p, 10, 1028, None) == EINVAL  # D > 1024
    assert lib.cvcl_layernorm_bwd_rows_f32(None, 768, p, p, 768, 1e-6, None, p, 768, p, 10, 768, None) == EINVAL
    assert lib.cvcl_gelu_f32(p, None, p, 6, None) == EINVAL
    assert lib.cvcl_gelu_f32(None, None, p, 8, None) == EINVAL
    assert lib.cvcl_vit_tokens_bwd_f32(p, p, p, 2, 1, 768, None) == EINVAL
    assert lib.cvcl_vit_tokens_bwd_f32(p, None, p, 2, 197, 768, None) == EINVAL
    nb = lib.cvcl_gemm_tn_colsum_f32_workspace_bytes(1000, 64, 64)
    assert nb > 0
    assert lib.cvcl_gemm_tn_colsum_f32(p, 64, p, 64, 1000, 64, 64, p, 65, p, p, nb, None) == EINVAL             # k_keep > K
    assert lib.cvcl_gemm_tn_colsum_f32(p, 32, p, 64, 1000, 64, 64, p, 64, p, p, nb, None) == EINVAL             # lda < N
    assert lib.cvcl_gemm_tn_colsum_f32(p, 64, p, 64, 1000, 64, 64, p, 64, p, p, nb - 4, None) == -3             # CVCL_EWORKSPACE
