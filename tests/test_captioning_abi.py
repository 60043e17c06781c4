"""CPU: the beam-search decoding surface -- the new entries declared, bound and exported with the ABI still at 7; their
refusals answer CVCL_EINVAL without a GPU; the captioning TextEncoder's parameters match the reference's state_dict keys; the
refusals of the model layer (attention, spatial features); the text-generation flags parse."""
import argparse
import contextlib
import io
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden

NEW = ("cvcl_beam_step", "cvcl_beam_finalize", "cvcl_lstm_cell_tok", "cvcl_lstm_cell_bwd_first")
FAKE = 1 << 20                 # a non-null stand-in pointer: every call below is refused before anything is dereferenced


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    return _hip


def test_declared_bound_exported_abi_7(H):
    hdr = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", hdr)
    assert re.search(r"CVCL_BEAM_MAX_K = 16, CVCL_BEAM_MAX_T = 128", hdr) and (H.BEAM_MAX_K, H.BEAM_MAX_T) == (16, 128)
    lib = H.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in H.SIGNATURES and hasattr(lib, name), name
    assert lib.cvcl_abi_version() == 7 == H.ABI_VERSION


def _step(lib, B=4, K=3, V=50, T=10, step=0, ptrs=None, alias=False):
    p = [FAKE + 256 * i for i in range(16)] if ptrs is None else ptrs
    a_in, a_out = p[1], (p[1] if alias else p[2])
    return lib.cvcl_beam_step(p[0], B, K, V, T, step, 0.6, 3, a_in, a_out, p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                              32, p[12], p[13], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(K=0), b"beam width"), (dict(K=17), b"beam width"), (dict(K=26, V=51), b"beam width"), (dict(K=4, V=7), b"2K"),
    (dict(T=0, step=0), b"decode length"), (dict(T=129), b"decode length"), (dict(step=10, T=10), b"bad sizes"),
    (dict(step=-1), b"bad sizes"), (dict(B=0), b"bad sizes"), (dict(ptrs=[FAKE] * 13 + [None] + [FAKE] * 2), b"null"),
    (dict(ptrs=[None] + [FAKE + 256 * i for i in range(1, 16)]), b"null"), (dict(alias=True), b"ping-pong")])
def test_beam_step_refusals(H, kw, msg):
    lib = H.load()
    assert _step(lib, **kw) == -1
    assert msg in lib.cvcl_last_error()


def test_finalize_and_cell_refusals(H):
    lib = H.load()
    f = FAKE
    assert lib.cvcl_beam_finalize(4, 0, 10, f, f, f, f, f, f, f, None) == -1
    assert lib.cvcl_beam_finalize(4, 17, 10, f, f, f, f, f, f, f, None) == -1
    assert lib.cvcl_beam_finalize(4, 3, 129, f, f, f, f, f, f, f, None) == -1
    assert lib.cvcl_beam_finalize(4, 3, 10, f, f, None, f, f, f, f, None) == -1 and b"null" in lib.cvcl_last_error()
    assert lib.cvcl_lstm_cell_tok(f, f, f, 50, f, f, 0, 32, None) == -1
    assert lib.cvcl_lstm_cell_tok(f, None, f, 50, f, f, 12, 32, None) == -1 and b"null" in lib.cvcl_last_error()
    assert lib.cvcl_lstm_cell_bwd_first(f, f, f, f, f, f, f, f, 0, 4, 32, None) == -1
    assert lib.cvcl_lstm_cell_bwd_first(f, f, None, f, f, f, f, f, 8, 4, 32, None) == -1 and b"null" in lib.cvcl_last_error()


def _args(**kw):
    a = dict(text_encoder="lstm", embedding_type="flat", embedding_dim=32, crange=1, dropout_i=0.0, dropout_o=0.0,
             pos_embed_type="no_pos_embed", captioning=True, attention=False, attention_gate=False, tie=True, bias=True)
    a.update(kw)
    return argparse.Namespace(**a)


def _text_encoder(**kw):
    from multimodal.multimodal import TextEncoder
    vocab = {"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, **{f"w{i}": i for i in range(4, 50)}}
    with contextlib.redirect_stdout(io.StringIO()):
        return TextEncoder(vocab, 2048, _args(**kw))


def test_captioning_state_dict_keys_match_reference():
    te = _text_encoder()
    ref = [str(k) for k in load_golden("captioning_beam")["state_dict_keys"]]
    assert sorted(te.state_dict()) == ref
    assert tuple(te.connector.weight.shape) == (64, 32) and tuple(te.connector.bias.shape) == (64,)
    assert not hasattr(_text_encoder(captioning=False), "connector")


def test_model_layer_refusals():
    from multimodal.multimodal import LanguageModel
    with pytest.raises(NotImplementedError):
        _text_encoder(attention=True)
    with pytest.raises(AssertionError):
        _text_encoder(text_encoder="transformer")                   # captioning needs the regressional (LSTM) encoder
    te = _text_encoder()
    with pytest.raises(NotImplementedError):                       # spatial features
        te.initial_state(torch.zeros(2, 32, 7, 7))
    lm = LanguageModel(te, _args())
    with pytest.raises(NotImplementedError):
        lm.beam_search_decode(2, 3, 10, 0.6, image_feature_map=torch.zeros(2, 32, 7, 7))
    plain = LanguageModel(_text_encoder(captioning=False), _args(captioning=False))
    with pytest.raises(ValueError):
        plain.beam_search_decode(2, 3, 10, 0.6, image_features=torch.zeros(2, 32))


def test_textgen_flags_parse():
    from multimodal.multimodal import TextEncoder
    from multimodal.multimodal_lit import MultiModalLitModel
    p = argparse.ArgumentParser()
    TextEncoder.add_to_argparse(p)
    MultiModalLitModel.add_to_argparse(p)
    a = p.parse_args(["--captioning", "--eval_textgen", "--beam_width", "5", "--decode_length", "20",
                      "--length_penalty_alpha", "0.7"])
    assert a.captioning and a.eval_textgen and (a.beam_width, a.decode_length, a.length_penalty_alpha) == (5, 20, 0.7)
