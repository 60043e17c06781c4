"""CPU: the alignment entries (cvcl_class_mean_f32, cvcl_cosine_matrix_f32, cvcl_triu_pearson_f32, cvcl_paired_l2_f32 and the two
workspace queries) are declared, bound and exported, refuse every invalid argument with CVCL_EINVAL on dummy pointers without
touching a GPU, and the Python layer refuses CPU tensors, non-fp32 tensors, label ids out of range, empty classes and unknown words."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_class_mean_f32", "cvcl_class_mean_workspace_bytes", "cvcl_cosine_matrix_f32", "cvcl_triu_pearson_f32",
           "cvcl_triu_pearson_workspace_bytes", "cvcl_paired_l2_f32")
FAKE = 0x10000                                          # 16-byte aligned, never dereferenced: validation fails first


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


def test_entries_declared_bound_exported(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    lib = H.lib()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name
    # the header cites the reference lines each entry replaces
    for cite in ("alignment.py:106-110", "alignment.py:148-161", "alignment.py:230-232", "embeddings.py:106-111",
                 "representation_similarity.py:5-12"):
        assert cite in txt, cite


def _mean(H, x=FAKE, label=FAKE, N=157, D=64, Cn=7, mean=FAKE, count=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return H.lib().cvcl_class_mean_f32(x, label, N, D, Cn, mean, count, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), b"null pointer (x / label)"),
    (dict(label=None), b"null pointer (x / label)"),
    (dict(mean=None), b"null pointer (mean / count)"),
    (dict(count=None), b"null pointer (mean / count)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(N=0), b"N 0 < 1"),
    (dict(N=-4), b"N -4 < 1"),
    (dict(N=1 << 24), b">= 2^24"),
    (dict(D=0), b"D 0 outside 1..2048"),
    (dict(D=2049), b"D 2049 outside 1..2048"),
    (dict(Cn=0), b"C 0 outside 1..4096"),
    (dict(Cn=4097), b"C 4097 outside 1..4096"),
    (dict(ws_bytes=16), b"workspace_bytes 16 <"),
    (dict(ws=FAKE + 4), b"not 16-byte aligned"),
])
def test_class_mean_refusals(H, kw, msg):
    assert _mean(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def _cos(H, a=FAKE, b=FAKE + 0x100000, M=22, K=22, D=512, eps=1e-8, out=FAKE):
    return H.lib().cvcl_cosine_matrix_f32(a, b, M, K, D, eps, out, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(a=None), b"null pointer (a / b)"),
    (dict(b=None), b"null pointer (a / b)"),
    (dict(out=None), b"null pointer (out)"),
    (dict(M=0), b"M 0 outside 1..4096"),
    (dict(M=4097), b"M 4097 outside 1..4096"),
    (dict(K=0), b"K 0 outside 1..4096"),
    (dict(K=4097), b"K 4097 outside 1..4096"),
    (dict(D=0), b"D 0 outside 1..2048"),
    (dict(D=2049), b"D 2049 outside 1..2048"),
    (dict(eps=-1.0), b"eps -1 < 0"),
    (dict(b=FAKE, K=23), b"a == b needs M == K"),
])
def test_cosine_matrix_refusals(H, kw, msg):
    assert _cos(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def _pearson(H, A=FAKE, B=FAKE, Cn=22, out=FAKE, ws=FAKE, ws_bytes=1 << 20):
    return H.lib().cvcl_triu_pearson_f32(A, B, Cn, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(A=None), b"null pointer (A / B)"),
    (dict(B=None), b"null pointer (A / B)"),
    (dict(out=None), b"null pointer (out)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(Cn=2), b"C 2 < 3"),
    (dict(Cn=0), b"C 0 < 3"),
    (dict(Cn=4097), b"C 4097 > 4096"),
    (dict(ws_bytes=8), b"workspace_bytes 8 <"),
    (dict(ws=FAKE + 8), b"not aligned"),
])
def test_pearson_refusals(H, kw, msg):
    assert _pearson(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def _l2(H, x=FAKE, y=FAKE, Cn=22, D=512, d=FAKE):
    return H.lib().cvcl_paired_l2_f32(x, y, Cn, D, 1e-6, d, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), b"null pointer (x / y)"),
    (dict(y=None), b"null pointer (x / y)"),
    (dict(d=None), b"null pointer (d)"),
    (dict(Cn=0), b"C 0 outside 1..4096"),
    (dict(Cn=4097), b"C 4097 outside 1..4096"),
    (dict(D=0), b"D 0 outside 1..2048"),
    (dict(D=2049), b"D 2049 outside 1..2048"),
])
def test_paired_l2_refusals(H, kw, msg):
    assert _l2(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def test_workspace_queries(H):
    lib = H.lib()
    qm, qp = lib.cvcl_class_mean_workspace_bytes, lib.cvcl_triu_pearson_workspace_bytes
    # the sorted row indices + one histogram row per chunk of rows + the class offsets; never an [N, D] copy
    assert 50000 * 4 + 2350 * 4 <= qm(50000, 512, 2350) < 50000 * 512
    assert qm(50000, 512, 2350) % 16 == 0 and qm(1, 1, 1) >= 16 + 16 + 16
    assert qm(0, 4, 4) == 0 and qm(4, 0, 4) == 0 and qm(4, 4, 0) == 0 and qm(1 << 24, 4, 4) == 0 and qm(4, 2049, 4) == 0
    assert qm((1 << 24) - 1, 2048, 4096) <= (1 << 24) * 4 + 256 * 4096 * 4 + 4096 * 4 + 48
    assert 0 < qp(3) <= qp(4096) <= 256 * 80 and qp(2) == 0 and qp(4097) == 0
    # the size the query gives is accepted as it is: the next check answers
    assert _mean(H, ws_bytes=qm(157, 64, 7), ws=FAKE + 4) == -1 and b"16-byte aligned" in lib.cvcl_last_error()
    assert _mean(H, ws_bytes=qm(157, 64, 7) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()
    assert _pearson(H, ws_bytes=qp(22), ws=FAKE + 8) == -1 and b"not aligned" in lib.cvcl_last_error()
    assert _pearson(H, ws_bytes=qp(22) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()


def test_python_layer_refusals(H):
    from multimodal import alignment as A
    x, t = torch.randn(12, 8), torch.randn(3, 8)
    lab = np.arange(12) % 3
    for call in (lambda: A.class_means(x, lab, 3), lambda: A.cosine_matrix(x), lambda: A.cosine_matrix(x, t),
                 lambda: A.cosine_dissim_matrix(x), lambda: A.rsa_of_dissim_matrices(t @ t.T, t @ t.T),
                 lambda: A.paired_distances(t, t), lambda: A.alignment(x, lab, t)):
        with pytest.raises(H.CvclError, match="device tensors"):          # CPU tensors: no fallback
            call()
    # dtype / shape / label checks need no device
    for bad in (torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.float32)):
        with pytest.raises(H.CvclError, match="fp32 rows"):               # non-fp32 / not [N, D]: refused wherever it lives
            A.cosine_matrix(bad)
        with pytest.raises(H.CvclError, match="fp32 rows"):
            A.class_means(bad, lab, 3)
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        A._labels(np.array([0, 1, 3]), 3, 3, "cpu")
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        A._labels(np.array([0, -1, 2]), 3, 3, "cpu")
    with pytest.raises(ValueError, match="integers"):
        A._labels(np.array([0.0, 1.0, 2.0]), 3, 3, "cpu")
    with pytest.raises(ValueError, match=r"must be \[4\]"):
        A._labels(np.array([0, 1, 2]), 4, 3, "cpu")
    with pytest.raises(ValueError, match=r"without a member: \[1, 3\]"):
        A._refuse_empty(np.array([4, 0, 2, 0]))
    A._refuse_empty(np.array([4, 1, 2]))
    vocab = {"ball": 71, "kitty": 76}
    with pytest.raises(KeyError, match="cat"):
        A.encode_words(None, ["ball", "cat"], vocab)                      # fails before the model is touched
    assert A.word_ids(["kitty", "ball"], vocab) == [76, 71]
