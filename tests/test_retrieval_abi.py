"""CPU: the retrieval-rank entries (cvcl_rank_cosine and its workspace query) are declared, bound and exported at ABI 7 and refuse
every invalid argument with CVCL_EINVAL on dummy pointers before anything reaches a GPU; the host side of multimodal/retrieval.py
(rank_summary, the key construction of image_text_retrieval, the refusal of a model that does not rank by cosine) on hand-written
cases."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from retrieval_common import pair_keys

ENTRIES = ("cvcl_rank_cosine", "cvcl_rank_cosine_workspace_bytes")
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
    assert len(H.SIGNATURES["cvcl_rank_cosine"][1]) == 18 and len(H.SIGNATURES["cvcl_rank_cosine_workspace_bytes"][1]) == 3


def _rank(H, q=FAKE, base=FAKE, ldq=64, ldb=64, Nq=10, Nb=20, D=64, eps=1e-8, qk=FAKE, bk=FAKE, thr_cos=FAKE, thr_idx=FAKE, off=0, acc=0,
          rank=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return H.lib().cvcl_rank_cosine(q, ldq, base, ldb, Nq, Nb, D, eps, qk, bk, thr_cos, thr_idx, off, acc, rank, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null pointer (q / base)"),
    (dict(base=None), b"null pointer (q / base)"),
    (dict(qk=None), b"null pointer (q_key / base_key)"),
    (dict(bk=None), b"null pointer (q_key / base_key)"),
    (dict(thr_cos=None), b"null pointer (thr_cos / thr_idx)"),
    (dict(thr_idx=None), b"null pointer (thr_cos / thr_idx)"),
    (dict(rank=None), b"null pointer (rank)"),
    (dict(ws=None), b"null pointer (workspace)"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(Nb=0), b"Nb 0 < 1"),
    (dict(Nb=-3), b"Nb -3 < 1"),
    (dict(D=0), b"D 0 < 1"),
    (dict(ldq=63), b"ldq 63 < D 64"),
    (dict(ldb=32), b"ldb 32 < D 64"),
    (dict(eps=-1.0), b"eps -1 < 0"),
    (dict(off=-1), b"idx_offset -1 < 0"),
    (dict(acc=2), b"accumulate 2 outside {0, 1}"),
    (dict(acc=-1), b"accumulate -1 outside {0, 1}"),
    (dict(ws_bytes=16), b"workspace_bytes 16 <"),
    (dict(ws=FAKE + 4), b"not 16-byte aligned"),
])
def test_rank_refusals(H, kw, msg):
    """each returns before the first launch: on a machine without a GPU a launch would fail with a runtime error instead"""
    assert _rank(H, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(b"cvcl_rank_cosine: ") and msg in err


def test_workspace_query(H):
    lib = H.lib()
    ws, nn = lib.cvcl_rank_cosine_workspace_bytes, lib.cvcl_nn_cosine_workspace_bytes
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, 0) == 0 and ws(-1, 5, 5) == 0
    assert ws(1, 1, 1) >= 16 + 16 + 4 and ws(3, 2, 33) % 16 == 0
    assert ws(10000, 10000, 512) == nn(10000, 10000, 512)                 # the arg-max search's layout
    assert (50000 + 50000) * 8 <= ws(50000, 50000, 512) < 50000 * 64 * 8    # norms + a few counts per query, never the matrix
    # the size the query gives is accepted as it is: the next check answers
    assert _rank(H, ws_bytes=ws(10, 20, 64), ws=FAKE + 4) == -1 and b"not 16-byte aligned" in lib.cvcl_last_error()
    assert _rank(H, ws_bytes=ws(10, 20, 64) - 1) == -1 and b"workspace_bytes" in lib.cvcl_last_error()


def test_python_layer_refuses_cpu_tensors_and_missing_keys(H):
    from multimodal import retrieval as R
    with pytest.raises(H.CvclError, match="device tensors"):
        R.retrieval_ranks(torch.randn(4, 8), torch.randn(6, 8), np.arange(4), np.arange(6))
    with pytest.raises(H.CvclError, match="device tensors"):
        R.image_text_retrieval(torch.randn(4, 8), torch.randn(4, 8), np.arange(4))


def test_rank_summary_on_hand_written_ranks(H):
    from multimodal import retrieval as R
    s = R.rank_summary(np.array([0, 4, -1, 9, 10, 0, 250, -1], dtype=np.int64), ks=(1, 5, 10), n_candidates=40)
    assert s["n_queries"] == 6 and s["n_without_positive"] == 2
    assert s["recall@1"] == 2 / 6 and s["recall@5"] == 3 / 6 and s["recall@10"] == 4 / 6
    assert s["median_rank"] == (5 + 10) / 2 and s["mean_rank"] == (1 + 5 + 10 + 11 + 1 + 251) / 6
    assert abs(s["mrr"] - (1 + 1 / 5 + 1 / 10 + 1 / 11 + 1 + 1 / 251) / 6) < 1e-15
    assert s["chance_recall@1"] == 1 / 40 and s["chance_recall@5"] == 5 / 40 and s["chance_recall@10"] == 10 / 40
    # ranks at or above every k; more k than candidates; a device-free tensor input
    s = R.rank_summary(torch.tensor([100, 200, 300]), ks=(1, 50), n_candidates=20)
    assert s["recall@1"] == 0.0 and s["recall@50"] == 0.0 and s["chance_recall@50"] == 1.0 and s["median_rank"] == 201.0
    assert "chance_recall@1" not in R.rank_summary(np.array([0, 1]))
    s = R.rank_summary(np.array([-1, -1]))
    assert s["n_queries"] == 0 and s["n_without_positive"] == 2 and math.isnan(s["recall@1"]) and math.isnan(s["median_rank"])
    with pytest.raises(ValueError):
        R.rank_summary(np.array([0.5, 1.0]))


def test_key_construction_on_six_pairs_with_two_repeated_utterances(H):
    from multimodal import retrieval as R
    tokens = np.array([[1, 7, 8, 2, 0], [1, 9, 2, 0, 0], [1, 7, 8, 2, 0], [1, 5, 2, 0, 0], [1, 9, 2, 0, 0], [1, 7, 8, 3, 2]])
    ids = R.text_ids_of(tokens)
    assert ids.dtype == np.int64 and ids[0] == ids[2] and ids[1] == ids[4] and len(set(ids.tolist())) == 4
    dense, first = R.retrieval_keys(ids)
    assert dense.tolist() == [0, 1, 0, 2, 1, 3] and first.tolist() == [0, 1, 3, 5]
    want = pair_keys(ids)
    assert np.array_equal(dense, want[0]) and np.array_equal(first, want[1])
    # ids in any numbering, as a tensor
    dense, first = R.retrieval_keys(torch.tensor([40, 7, 40, 7, 7, 3]))
    assert dense.tolist() == [0, 1, 0, 1, 1, 2] and first.tolist() == [0, 1, 5]
    # rows are compared whole, padding included: a shorter utterance is another text
    assert R.text_ids_of(np.array([[1, 4, 2], [1, 4, 0], [1, 4, 2]])).tolist() == [1, 0, 1]


def test_a_model_that_does_not_normalise_is_refused(H):
    from multimodal import retrieval as R
    off = types.SimpleNamespace(normalize_features=False, embedding_type="flat")
    with pytest.raises(H.CvclError, match="normalize_features off"):
        R.require_cosine_model(off)
    with pytest.raises(H.CvclError, match="normalize_features off"):
        R.require_cosine_model(types.SimpleNamespace(model=off))          # a lit model wraps the two-tower model
    R.require_cosine_model(types.SimpleNamespace(normalize_features=True, embedding_type="flat"))
    with pytest.raises(H.CvclError, match="embedding_type"):
        R.require_cosine_model(types.SimpleNamespace(normalize_features=True, embedding_type="spatial"))
