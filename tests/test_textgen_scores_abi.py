"""CPU: the caption-score entries (cvcl_caption_bleu_rouge, cvcl_caption_ref_keys, cvcl_caption_cider) are declared, bound and
exported at ABI 7 and refuse every argument outside their limits with CVCL_EINVAL on dummy pointers without touching a GPU;
textgen_eval.evaluate has the reference's parameter list, and neither it nor ops.caption_scores has a CPU path."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_caption_bleu_rouge", "cvcl_caption_ref_keys", "cvcl_caption_cider")
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


def test_entries_declared_bound_exported_at_abi_7(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    lib = H.lib()
    assert lib.cvcl_abi_version() == H.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name
    assert (H.CAPTION_MAX_LEN, H.CAPTION_MAX_REFS, H.CAPTION_ORDERS) == (128, 32, 4) and H.CAPTION_SENTINEL < 0
    assert [len(H.SIGNATURES[n][1]) for n in ENTRIES] == [15, 10, 17]


def _call(H, entry, hyp=FAKE, hyp_len=FAKE, N=3, Lh=6, ref=FAKE, ref_len=FAKE, R=5, Lr=7, off=(0, 2, 3, 5), off_dev=FAKE, V=30,
          stats=FAKE, rouge=FAKE, bad=FAKE, keys=FAKE, df_key=FAKE, df_cnt=FAKE, df_off=(0, 4, 9, 12, 13), n_df=13, cider=FAKE):
    arr = lambda v: None if v is None else (C.c_int64 * len(v))(*v)              # noqa: E731
    corpus = (ref, ref_len, R, Lr, arr(off), off_dev, V)
    if entry == "cvcl_caption_bleu_rouge":
        return H.lib().cvcl_caption_bleu_rouge(hyp, hyp_len, N, Lh, *corpus, stats, rouge, bad, None)
    if entry == "cvcl_caption_ref_keys":
        return H.lib().cvcl_caption_ref_keys(ref, ref_len, N, *corpus[2:], keys, None)
    return H.lib().cvcl_caption_cider(hyp, hyp_len, N, Lh, *corpus, df_key, df_cnt, arr(df_off), n_df, cider, None)


CORPUS_REFUSALS = [
    (dict(Lr=129), b"Lr 129 outside 1..128 tokens per sentence"),
    (dict(Lr=0), b"Lr 0 outside 1..128"),
    (dict(off=(0, 0, 3, 5)), b"example 0 has 0 references (outside 1..32)"),
    (dict(off=(0, 2, 2, 5)), b"example 1 has 0 references"),
    (dict(off=(0, 4, 3, 5)), b"ref_off decreases at example 1"),
    (dict(N=2, R=40, off=(0, 33, 40)), b"example 0 has 33 references (outside 1..32)"),
    (dict(off=(1, 2, 3, 5)), b"ref_off must run from 0 to R 5"),
    (dict(off=(0, 2, 3, 4)), b"ref_off must run from 0 to R 5"),
    (dict(V=32769), b"4 x 16 bits per token (vocab_size 32769) > 63 key bits"),
    (dict(V=0), b"vocab_size 0 < 1"),
    (dict(N=0), b"N 0 < 1"),
    (dict(R=0), b"R 0 references"),
    (dict(ref=None), b"null pointer (ref / ref_len / ref_off / ref_off_dev)"),
    (dict(ref_len=None), b"null pointer (ref / ref_len / ref_off / ref_off_dev)"),
    (dict(off=None), b"null pointer (ref / ref_len / ref_off / ref_off_dev)"),
    (dict(off_dev=None), b"null pointer (ref / ref_len / ref_off / ref_off_dev)"),
]
HYP_REFUSALS = [
    (dict(Lh=129), b"Lh 129 outside 1..128 tokens per sentence"),
    (dict(Lh=0), b"Lh 0 outside 1..128"),
    (dict(hyp=None), b"null pointer (hyp / hyp_len)"),
    (dict(hyp_len=None), b"null pointer (hyp / hyp_len)"),
]


def _refused(H, entry, kw, msg):
    assert _call(H, entry, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(entry.encode() + b": ") and msg in err, err


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,msg", CORPUS_REFUSALS)
def test_corpus_refusals(H, entry, kw, msg):
    _refused(H, entry, kw, msg)


@pytest.mark.parametrize("entry", (ENTRIES[0], ENTRIES[2]))
@pytest.mark.parametrize("kw,msg", HYP_REFUSALS)
def test_hypothesis_refusals(H, entry, kw, msg):
    _refused(H, entry, kw, msg)


@pytest.mark.parametrize("entry,kw,msg", [
    (ENTRIES[0], dict(stats=None), b"null pointer (stats / rouge / bad)"),
    (ENTRIES[0], dict(rouge=None), b"null pointer (stats / rouge / bad)"),
    (ENTRIES[0], dict(bad=None), b"null pointer (stats / rouge / bad)"),
    (ENTRIES[1], dict(keys=None), b"null pointer (keys)"),
    (ENTRIES[2], dict(df_off=None), b"null pointer (df_off)"),
    (ENTRIES[2], dict(df_off=(1, 4, 9, 12, 13)), b"df_off must run from 0 to n_df 13"),
    (ENTRIES[2], dict(n_df=14), b"df_off must run from 0 to n_df 14"),
    (ENTRIES[2], dict(df_off=(0, 10, 9, 12, 13)), b"df_off decreases at order 2"),
    (ENTRIES[2], dict(df_key=None), b"null pointer (df_key / df_cnt)"),
    (ENTRIES[2], dict(df_cnt=None), b"null pointer (df_key / df_cnt)"),
    (ENTRIES[2], dict(cider=None), b"null pointer (cider)"),
])
def test_output_and_table_refusals(H, entry, kw, msg):
    _refused(H, entry, kw, msg)


def test_the_limits_themselves_are_accepted_up_to_the_pointers(H):
    """128 tokens, 32 references and vocab_size 32768 pass the limit checks: the refusal that follows names a later argument."""
    for entry in ENTRIES:
        _refused(H, entry, dict(Lh=128, Lr=128, N=2, R=33, off=(0, 32, 33), V=32768, stats=None, keys=None, cider=None), b"null pointer (")


def test_evaluate_has_the_reference_parameter_list(H):
    from multimodal import textgen_eval
    sig = inspect.signature(textgen_eval.evaluate)
    assert list(sig.parameters) == ["list_of_references", "hypotheses", "keys"] and sig.parameters["keys"].default is None
    with pytest.raises(ValueError, match="2 reference entries for 1 hypotheses"):
        textgen_eval.evaluate(["a", "b"], ["a"])
    with pytest.raises(ValueError, match="at least one"):
        textgen_eval.evaluate([], [])


def test_no_cpu_fallback(H):
    from multimodal import ops, textgen_eval
    i64 = torch.int64
    hyp, ref = torch.zeros(2, 3, dtype=i64), torch.zeros(3, 4, dtype=i64)
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        ops.caption_scores(hyp, torch.tensor([3, 2]), ref, torch.tensor([4, 1, 2]), torch.tensor([0, 1, 3]), 5)
    with pytest.raises(ValueError, match="one length per sentence"):
        ops.caption_scores(hyp, torch.tensor([3]), ref, torch.tensor([4, 1, 2]), torch.tensor([0, 1, 3]), 5)
    if not torch.cuda.is_available():
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            textgen_eval.evaluate(["a b"], ["a"])
