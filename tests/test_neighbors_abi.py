"""CPU: the nearest-neighbour entries (cvcl_nn_cosine, cvcl_nn_l1_u8 and their workspace queries) are declared, bound and exported at
ABI 7, refuse every invalid argument with CVCL_EINVAL on dummy pointers without touching a GPU, and the Python layer refuses CPU
tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_nn_cosine", "cvcl_nn_cosine_workspace_bytes", "cvcl_nn_l1_u8", "cvcl_nn_l1_u8_workspace_bytes")
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


def _cosine(H, q=FAKE, base=FAKE, ldq=64, ldb=64, Nq=10, Nb=20, D=64, qg=None, bg=None, off=0, cos=FAKE, idx=FAKE, ws=FAKE,
            ws_bytes=1 << 30):
    return H.lib().cvcl_nn_cosine(q, ldq, base, ldb, Nq, Nb, D, 1e-8, qg, bg, off, 0, cos, idx, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null pointer (q / base)"),
    (dict(base=None), b"null pointer (q / base)"),
    (dict(cos=None), b"null pointer (best_cos / best_idx)"),
    (dict(idx=None), b"null pointer (best_cos / best_idx)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(Nb=0), b"Nb 0 < 1"),
    (dict(Nb=-3), b"Nb -3 < 1"),
    (dict(D=0), b"D 0 < 1"),
    (dict(ldq=63), b"ldq 63 < D 64"),
    (dict(ldb=32), b"ldb 32 < D 64"),
    (dict(qg=FAKE), b"go together"),
    (dict(bg=FAKE), b"go together"),
    (dict(off=-1), b"idx_offset -1 < 0"),
    (dict(ws_bytes=16), b"workspace_bytes 16 <"),
    (dict(ws=FAKE + 4), b"not 16-byte aligned"),
])
def test_cosine_refusals(H, kw, msg):
    assert _cosine(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def _pixels(H, q=FAKE, base=FAKE, Nq=4, Nb=9, Cn=3, HW=64, w=True, qg=None, bg=None, off=0, dist=FAKE, idx=FAKE, sums=None, ws=FAKE,
            ws_bytes=1 << 30):
    warr = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0) if w else None
    return H.lib().cvcl_nn_l1_u8(q, base, Nq, Nb, Cn, HW, warr, qg, bg, off, 0, dist, idx, sums, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null pointer (q / base)"),
    (dict(base=None), b"null pointer (q / base)"),
    (dict(w=False), b"null pointer (w)"),
    (dict(dist=None), b"null pointer (best_dist / best_idx)"),
    (dict(idx=None), b"null pointer (best_dist / best_idx)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(Nb=0), b"Nb 0 < 1"),
    (dict(Cn=0), b"C 0 outside 1..4"),
    (dict(Cn=5), b"C 5 outside 1..4"),
    (dict(HW=0), b"HW 0 is not a positive multiple of 4"),
    (dict(HW=66), b"HW 66 is not a positive multiple of 4"),
    (dict(HW=16843012), b"can exceed 32 bits"),                 # 16843012 * 255 >= 2^32
    (dict(q=FAKE + 2), b"not 4-byte aligned"),
    (dict(qg=FAKE), b"go together"),
    (dict(bg=FAKE), b"go together"),
    (dict(off=-5), b"idx_offset -5 < 0"),
    (dict(ws_bytes=8), b"workspace_bytes 8 <"),
    (dict(ws=FAKE + 8), b"not 16-byte aligned"),
])
def test_pixel_refusals(H, kw, msg):
    assert _pixels(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def test_workspace_queries(H):
    lib = H.lib()
    qc, qp = lib.cvcl_nn_cosine_workspace_bytes, lib.cvcl_nn_l1_u8_workspace_bytes
    # norms of both sides in double + at least one (value, index) partial per query; never a queries x base matrix
    assert (2200 + 50000) * 8 + 2200 * 8 <= qc(2200, 50000, 2048) < 2200 * 50000
    assert qc(2200, 50000, 2048) % 16 == 0 and qc(1, 1, 1) >= 16 + 16 + 8
    assert qc(0, 5, 5) == 0 and qc(5, 0, 5) == 0 and qc(5, 5, 0) == 0
    assert 2200 * (8 + 4 + 12) <= qp(2200, 50000, 3) < 2200 * 50000
    assert qp(4, 4, 0) == 0 and qp(4, 4, 5) == 0 and qp(0, 4, 3) == 0
    # the size the query gives is accepted as it is: the next check (here the group pair) answers
    assert _cosine(H, ws_bytes=qc(10, 20, 64), qg=FAKE) == -1 and b"go together" in lib.cvcl_last_error()
    assert _cosine(H, ws_bytes=qc(10, 20, 64) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()
    assert _pixels(H, ws_bytes=qp(4, 9, 3), qg=FAKE) == -1 and b"go together" in lib.cvcl_last_error()
    assert _pixels(H, ws_bytes=qp(4, 9, 3) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()


def test_python_layer_refuses_cpu_tensors(H):
    from multimodal import neighbors as N
    with pytest.raises(H.CvclError):
        N.nearest_cosine(torch.randn(4, 8), torch.randn(6, 8))
    with pytest.raises(H.CvclError):
        N.nearest_pixels(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(5, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(H.CvclError):
        N.extract_features(torch.nn.Identity(), torch.zeros(2, 3, 32, 32))
