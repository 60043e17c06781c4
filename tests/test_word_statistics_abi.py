"""CPU: the word-statistics entries (cvcl_token_items_accumulate, cvcl_token_topk) are declared, bound and exported and refuse
invalid arguments with CVCL_EINVAL on dummy pointers without touching a GPU; analysis_tools.processing imports and exposes the
reference's names."""
import os
import re

import pytest

from conftest import ROOT

ENTRIES = ("cvcl_token_items_accumulate", "cvcl_token_topk")
FAKE = 0x10000                                          # never dereferenced: validation fails first


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
    assert lib.cvcl_abi_version() == H.ABI_VERSION == int(re.search(r"#define CVCL_ABI_VERSION (\d+)", txt).group(1))
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "processing.py:326-331" in txt and "processing.py:352" in txt and "utils.py:142" in txt   # the reference lines replaced
    assert H.TOKEN_TOPK_MAX_K == int(re.search(r"CVCL_TOKEN_TOPK_MAX_K = (\d+)", txt).group(1)) == 16


def _acc(H, outputs=FAKE, loss=FAKE, N=8, Hd=5, seg=FAKE, rows=FAKE, slot=FAKE, S=2, n_valid=6, vec=FAKE, ls=FAKE, cnt=FAKE, K=4):
    return H.lib().cvcl_token_items_accumulate(outputs, loss, N, Hd, seg, rows, slot, S, n_valid, vec, ls, cnt, K, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(outputs=None), b"null pointer"), (dict(loss=None), b"null pointer"), (dict(seg=None), b"null pointer"),
    (dict(rows=None), b"null pointer"), (dict(slot=None), b"null pointer"), (dict(vec=None), b"null pointer"),
    (dict(ls=None), b"null pointer"), (dict(cnt=None), b"null pointer"),
    (dict(N=0), b"bad sizes"), (dict(Hd=0), b"bad sizes"), (dict(K=0), b"bad sizes"), (dict(S=-1), b"bad sizes"),
    (dict(S=5), b"5 segments for 4 keys"), (dict(n_valid=1), b"1 rows for 2 segments"),
])
def test_accumulate_refusals(H, kw, msg):
    assert _acc(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def test_accumulate_empty_batch_is_a_no_op(H):
    assert _acc(H, S=0, n_valid=0) == 0                  # nothing is enqueued: no GPU is touched


def _topk(H, logits=FAKE, labels=FAKE, R=4, V=50, k=5, tp=FAKE, ti=FAKE, lp=FAKE, probs=None):
    return H.lib().cvcl_token_topk(logits, labels, R, V, k, 0, tp, ti, lp, probs, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(tp=None), b"null pointer"),
    (dict(ti=None), b"null pointer"), (dict(lp=None), b"null pointer"),
    (dict(k=0), b"k 0 outside [1, 16]"), (dict(k=17), b"k 17 outside [1, 16]"),
    (dict(V=4), b"vocabulary size 4 outside [k = 5, 12288]"), (dict(V=12289), b"vocabulary size 12289 outside"),
    (dict(R=0), b"bad row count"), (dict(probs=FAKE), b"must not alias"),
])
def test_topk_refusals(H, kw, msg):
    assert _topk(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error()


def test_analysis_tools_import_path(H):
    from analysis_tools import processing as P
    from analysis_tools import sumdata, token_items_data, utils
    for name in ("is_regressional", "run_model", "run_model_on_batches", "run_model_on_data", "get_model_losses_on_batches",
                 "get_model_items", "get_token_items", "update_items_with_embedding", "get_model_probs", "get_model_top_predictions",
                 "build_series", "build_series_from_pairs", "ModelItems"):
        assert hasattr(P, name), name
    assert P.ModelItems._fields == ("losses", "all_token_items", "token_pos_items", "token_items")
    assert token_items_data.Key._fields == ("token_id", "pos") and P.Key is token_items_data.Key
    assert P.SumData is sumdata.SumData and callable(utils.print_top_values) and callable(utils.get_model_device)
