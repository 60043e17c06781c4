"""CPU: the k-nearest-neighbour entries (cvcl_knn_cosine, its workspace query, cvcl_knn_vote) and their two limits are declared, bound
and exported at ABI 7, refuse every invalid argument with CVCL_EINVAL on dummy pointers without touching a GPU, and the Python layer
refuses CPU tensors and k outside 1..256."""
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_knn_cosine", "cvcl_knn_cosine_workspace_bytes", "cvcl_knn_vote")
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


def test_entries_declared_bound_exported_at_abi_7(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt)
    lib = H.lib()
    assert lib.cvcl_abi_version() == 7 == H.ABI_VERSION
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define CVCL_KNN_MAX_K 256\b", txt) and H.KNN_MAX_K == 256
    assert re.search(r"#define CVCL_KNN_MAX_CLASSES 4096\b", txt) and H.KNN_MAX_CLASSES == 4096
    assert len(H.SIGNATURES["cvcl_knn_cosine"][1]) == 18 and len(H.SIGNATURES["cvcl_knn_vote"][1]) == 11


def _search(H, q=FAKE, base=FAKE, ldq=64, ldb=64, Nq=10, Nb=20, D=64, k=5, qg=None, bg=None, off=0, cos=FAKE, idx=FAKE, ws=FAKE,
            ws_bytes=1 << 30):
    return H.lib().cvcl_knn_cosine(q, ldq, base, ldb, Nq, Nb, D, k, 1e-8, qg, bg, off, 0, cos, idx, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null pointer (q / base)"),
    (dict(base=None), b"null pointer (q / base)"),
    (dict(cos=None), b"null pointer (top_cos / top_idx)"),
    (dict(idx=None), b"null pointer (top_cos / top_idx)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(Nb=0), b"Nb 0 < 1"),
    (dict(Nb=-3), b"Nb -3 < 1"),
    (dict(D=0), b"D 0 < 1"),
    (dict(k=0), b"k 0 outside 1..256"),
    (dict(k=-1), b"k -1 outside 1..256"),
    (dict(k=257), b"k 257 outside 1..256"),
    (dict(ldq=63), b"ldq 63 < D 64"),
    (dict(ldb=32), b"ldb 32 < D 64"),
    (dict(qg=FAKE), b"go together"),
    (dict(bg=FAKE), b"go together"),
    (dict(off=-1), b"idx_offset -1 < 0"),
    (dict(ws_bytes=16), b"workspace_bytes 16 <"),
    (dict(ws=FAKE + 4), b"not 16-byte aligned"),
])
def test_search_refusals(H, kw, msg):
    assert _search(H, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(b"cvcl_knn_cosine: ") and msg in err


def _vote(H, cos=FAKE, idx=FAKE, Nq=4, k=5, lab=FAKE, Nb=9, Cn=3, T=0.07, scores=FAKE, pred=FAKE):
    return H.lib().cvcl_knn_vote(cos, idx, Nq, k, lab, Nb, Cn, T, scores, pred, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(cos=None), b"null pointer (top_cos / top_idx)"),
    (dict(idx=None), b"null pointer (top_cos / top_idx)"),
    (dict(lab=None), b"null pointer (base_label)"),
    (dict(scores=None), b"null pointer (scores / pred)"),
    (dict(pred=None), b"null pointer (scores / pred)"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(k=0), b"k 0 outside 1..256"),
    (dict(k=300), b"k 300 outside 1..256"),
    (dict(Cn=0), b"C 0 outside 1..4096"),
    (dict(Cn=4097), b"C 4097 outside 1..4096"),
    (dict(Nb=0), b"Nb 0 < 1"),
    (dict(Nb=-7), b"Nb -7 < 1"),
    (dict(T=-0.5), b"temperature -0.5 is negative or not finite"),
    (dict(T=float("inf")), b"temperature inf is negative or not finite"),
    (dict(T=float("nan")), b"is negative or not finite"),
])
def test_vote_refusals(H, kw, msg):
    assert _vote(H, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(b"cvcl_knn_vote: ") and msg in err


def test_workspace_query(H):
    lib = H.lib()
    ws, nn = lib.cvcl_knn_cosine_workspace_bytes, lib.cvcl_nn_cosine_workspace_bytes
    sizes = [ws(2200, 50000, 2048, k) for k in (1, 2, 20, 64, 200, 256)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)          # grows with k, 16-byte granular
    assert ws(2200, 50000, 2048, 1) == nn(2200, 50000, 2048)                    # one (value, row) pair per (split, query): the arg-max's
    # the norms of both sides in double + at least one list of k pairs per query; never the queries x base matrix
    assert (2200 + 50000) * 8 + 2200 * 20 * 8 <= ws(2200, 50000, 2048, 20) < 2200 * 50000 * 4
    assert ws(1, 1, 1, 1) >= 16 + 16 + 8 and ws(3, 2, 33, 5) % 16 == 0
    assert ws(0, 5, 5, 1) == 0 and ws(5, 0, 5, 1) == 0 and ws(5, 5, 0, 1) == 0 and ws(5, 5, 5, 0) == 0 and ws(5, 5, 5, 257) == 0
    # the size the query gives is accepted as it is: the next check (here the group pair) answers
    assert _search(H, ws_bytes=ws(10, 20, 64, 5), qg=FAKE) == -1 and b"go together" in lib.cvcl_last_error()
    assert _search(H, ws_bytes=ws(10, 20, 64, 5) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()


def test_python_layer_refuses_cpu_tensors_and_k_out_of_range(H):
    from multimodal import neighbors as N
    with pytest.raises(H.CvclError, match="device tensors"):
        N.knn_cosine(torch.randn(4, 8), torch.randn(6, 8), 3)
    for k in (0, -2, 257):
        with pytest.raises(H.CvclError, match=f"k {k} outside 1..256"):
            N.knn_cosine(torch.randn(4, 8), torch.randn(6, 8), k)
    with pytest.raises(H.CvclError, match="device tensors"):
        N.knn_vote(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), 2)
    with pytest.raises(H.CvclError, match="device tensors"):
        N.knn_classify(torch.randn(4, 8), ["a"] * 4, torch.randn(6, 8), ["a"] * 6, k=3)
