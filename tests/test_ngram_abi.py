"""CPU: the n-gram entries (cvcl_ngram_keys, cvcl_ngram_ce_loss, cvcl_ngram_probs) are declared, bound and exported at ABI 7 and
refuse every invalid argument with CVCL_EINVAL on dummy pointers without touching a GPU; ngram.NGramModel refuses bad N,
vocab_size and alpha with ValueError before any launch and has no CPU fallback; analysis_tools.processing still refuses
``model is None`` and an object that only carries the name NGramModel."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("cvcl_ngram_keys", "cvcl_ngram_ce_loss", "cvcl_ngram_probs")
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
    assert lib.cvcl_abi_version() == H.ABI_VERSION == int(re.search(r"#define CVCL_ABI_VERSION (\d+)", txt).group(1)) == 7
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES, name
        assert hasattr(lib, name), name
    assert H.NGRAM_MAX_N == int(re.search(r"CVCL_NGRAM_MAX_N = (\d+)", txt).group(1)) == 8 and H.NGRAM_SENTINEL < 0
    assert len(H.SIGNATURES["cvcl_ngram_keys"][1]) == 9
    assert H.SIGNATURES["cvcl_ngram_ce_loss"] == H.SIGNATURES["cvcl_ngram_probs"] and len(H.SIGNATURES["cvcl_ngram_probs"][1]) == 19
    assert "not normalised" in re.sub(r"\s+", " ", txt.lower().replace("*", ""))           # the header says what the probabilities are


MODEL_REFUSALS = [
    (dict(N=0), b"N 0 outside 1..8"),
    (dict(N=9), b"N 9 outside 1..8"),
    (dict(N=-1), b"N -1 outside 1..8"),
    (dict(V=0), b"vocab_size 0 < 1"),
    (dict(V=-5), b"vocab_size -5 < 1"),
    (dict(N=5, V=4097), b"N 5 x 13 bits per token (vocab_size 4097) > 63 key bits"),
    (dict(N=4, V=65536), b"N 4 x 16 bits per token (vocab_size 65536) > 63 key bits"),
    (dict(B=-1), b"B -1 < 0"),
    (dict(L=0), b"L 0 < 1"),
    (dict(B=1 << 20, L=1 << 11), b"do not fit 31 bits"),
]


def _keys(H, y=FAKE, y_len=FAKE, B=4, L=6, N=3, V=30, keys=FAKE, bad=FAKE):
    return H.lib().cvcl_ngram_keys(y, y_len, B, L, N, V, keys, bad, None)


@pytest.mark.parametrize("kw,msg", MODEL_REFUSALS + [
    (dict(y=None), b"null pointer (y / y_len / keys)"),
    (dict(y_len=None), b"null pointer (y / y_len / keys)"),
    (dict(keys=None), b"null pointer (y / y_len / keys)"),
    (dict(bad=None), b"null pointer (bad)"),
])
def test_keys_refusals(H, kw, msg):
    assert _keys(H, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(b"cvcl_ngram_keys: ") and msg in err


def _score(H, entry, gk=FAKE, gc=FAKE, goff=(0, 5, 12, 20), n_gram=20, ck=FAKE, ct=FAKE, coff=(0, 1, 4, 9), n_ctx=9, N=3, V=30,
           la=-2.3, l1a=-0.1, y=FAKE, y_len=FAKE, B=4, L=6, out=FAKE, bad=FAKE):
    arr = lambda v: None if v is None else (C.c_int64 * len(v))(*v)              # noqa: E731
    return getattr(H.lib(), entry)(gk, gc, arr(goff), n_gram, ck, ct, arr(coff), n_ctx, N, V, la, l1a, y, y_len, B, L, out, bad, None)


TABLE_REFUSALS = [
    (dict(goff=None), b"null pointer (gram_off / ctx_off)"),
    (dict(coff=None), b"null pointer (gram_off / ctx_off)"),
    (dict(n_gram=-1), b"negative table size"),
    (dict(goff=(1, 5, 12, 20)), b"gram_off must run from 0 to n_gram 20"),
    (dict(n_gram=21), b"gram_off must run from 0 to n_gram 21"),
    (dict(coff=(0, 1, 4, 8)), b"ctx_off must run from 0 to n_ctx 9"),
    (dict(goff=(0, 13, 12, 20)), b"decrease at order 1"),
    (dict(coff=(0, 1, 0, 9)), b"decrease at order 1"),
    (dict(coff=(0, 1, 9, 9)), b"order 1 has 8 contexts for 7 grams"),
    (dict(coff=(0, 1, 1, 9)), b"order 1 has 0 contexts for 7 grams"),
    (dict(coff=(0, 2, 4, 9)), b"order 0 has 2 contexts"),
    (dict(gk=None), b"null pointer (gram_key / gram_cnt / ctx_key / ctx_tot)"),
    (dict(gc=None), b"null pointer (gram_key / gram_cnt / ctx_key / ctx_tot)"),
    (dict(ck=None), b"null pointer (gram_key / gram_cnt / ctx_key / ctx_tot)"),
    (dict(ct=None), b"null pointer (gram_key / gram_cnt / ctx_key / ctx_tot)"),
    (dict(la=0.5), b"is positive or NaN"),
    (dict(l1a=float("nan")), b"is positive or NaN"),
    (dict(bad=None), b"null pointer (bad)"),
    (dict(y=None), b"null pointer (y / y_len"),
    (dict(y_len=None), b"null pointer (y / y_len"),
    (dict(out=None), b"null pointer"),
]


@pytest.mark.parametrize("entry", ENTRIES[1:])
@pytest.mark.parametrize("kw,msg", MODEL_REFUSALS + TABLE_REFUSALS)
def test_score_refusals(H, entry, kw, msg):
    assert _score(H, entry, **kw) == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(entry.encode() + b": ") and msg in err


def test_probs_needs_a_position(H):
    for kw in (dict(B=0), dict(L=1)):
        assert _score(H, "cvcl_ngram_probs", **kw) == -1 and b"no position to score" in H.lib().cvcl_last_error()


def test_class_refusals_before_any_launch(H):
    from ngram import NGramModel, key_bits
    assert [key_bits(v) for v in (1, 2, 3, 7, 2350, 4096, 4097, 65536)] == [1, 1, 2, 3, 12, 12, 13, 16]
    for N, V in ((0, 30), (9, 30), (-1, 30), (2.5, 30), (3, 0), (3, -2), (5, 4097), (4, 65536), (6, 2350)):
        with pytest.raises(ValueError):
            NGramModel(N, V)
    assert NGramModel(5, 2350).N == 5 and NGramModel(5, 4096).vocab_size == 4096 and NGramModel(8, 128).N == 8
    model = NGramModel(3, 30)
    y, y_len = torch.tensor([[1, 4, 2]]), torch.tensor([3])
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            model.calculate_ce_loss(y, y_len, alpha=alpha)
        with pytest.raises(ValueError, match="alpha"):
            model.calculate_probs(y, y_len, alpha=alpha)


def test_no_cpu_fallback(H):
    """A model on the CPU is refused, with or without a GPU in the machine; so are CPU tensors handed to the wrappers."""
    from analysis_tools import processing as P
    from multimodal import ops
    from ngram import NGramModel
    y, y_len = torch.tensor([[1, 4, 2]]), torch.tensor([3])
    models = [NGramModel(3, 30, device="cpu")] + ([] if torch.cuda.is_available() else [NGramModel(3, 30)])
    for model in models:
        for fn in (model.update, model.calculate_ce_loss, model.calculate_probs):
            with pytest.raises(H.CvclError, match="no CPU fallback"):
                fn(y, y_len)
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            model.to_counts()
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            P.run_model(model, y, y_len)
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        P.build_ngram_model(3, 30, [(None, y, y_len, None)], device="cpu")
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        ops.ngram_keys(y, y_len, 3, 30)
    empty = torch.zeros(0, dtype=torch.int64)
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        ops.ngram_ce_loss((empty, empty, [0] * 4, empty, empty, [0] * 4), 3, 30, -2.3, -0.1, y, y_len)


def test_processing_refusals_are_unchanged(H):
    from analysis_tools import processing as P
    y, ln = torch.tensor([[2, 5, 3]]), torch.tensor([3])

    class NGramModel:
        pass

    for bad, msg in ((None, "model is None"), (NGramModel(), "n-gram models are outside")):
        with pytest.raises(NotImplementedError, match=msg):
            P.run_model(bad, y, ln)
        with pytest.raises(NotImplementedError, match=msg):
            P.get_model_items(bad, [(None, y, ln, None)], [[".", "NN", "."]])
        with pytest.raises(NotImplementedError, match=msg):
            P.get_model_top_predictions(bad, [(None, y, ln, None)], [[".", "NN", "."]])
    assert P.is_regressional(None) is False
    from ngram import NGramModel as Real
    assert P.is_regressional(Real(3, 30)) is True
    for name in ("build_ngram_model", "run_model", "get_model_items", "get_model_probs", "get_model_top_predictions"):
        assert callable(getattr(P, name))
