"""GPU: the caption scores of csrc/textgen_scores.hip (ops.caption_scores, textgen_eval.evaluate) against the float64 restatement of
tests/textgen_scores_common.py on seeded corpora, their determinism and refusals, and the Lightning wiring that logs them.

The bound on every floating-point number is a relative 1e-11 (plus an absolute 1e-15 where one side is exactly 0): every sum is of
at most a few thousand non-negative double terms, and the only cancellation, log N - log df, is at least log(65 / 64) at N <= 65,
so the expected error is near 1e-13.  The integer statistics and the document-frequency tables must be equal exactly."""
import argparse
import contextlib
import io
import os
import sys
import types

import pytest
import torch

import textgen_scores_common as TC
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [(n, vocab) for n in (1, 2, 7, 65) for vocab in (5, 300)]
_cache = {}


def _case(dev, n, vocab):
    """(corpus, the restatement's result, the device's result, the device tensors), computed once per case"""
    if (n, vocab) not in _cache:
        from multimodal import ops
        hyps, refs = TC.corpus(n, n, vocab)
        t = TC.tensors(hyps, refs, dev)
        _cache[n, vocab] = ((hyps, refs), TC.score_corpus(hyps, refs), ops.caption_scores(*t, vocab), t)
    return _cache[n, vocab]


def rel_err(got, want):
    """0 when the pair is within the absolute 1e-15 allowed where one side is exactly 0, else the relative error"""
    if got == want or ((got == 0.0 or want == 0.0) and abs(got - want) <= 1e-15):
        return 0.0
    return abs(got - want) / max(abs(got), abs(want))


@pytest.mark.parametrize("n,vocab", CASES)
def test_scores_match_the_restatement(dev, n, vocab):
    (hyps, refs), (want, want_arrays), (got, arrays), _t = _case(dev, n, vocab)
    assert arrays["stats"].tolist() == want_arrays["stats"]
    for order in range(1, 5):
        keys, counts = arrays["df"][order - 1]
        assert torch.equal(keys, torch.sort(keys).values) and TC.unpack_df(keys, counts, order, vocab) == want_arrays["df"][order - 1]
    assert tuple(got) == TC.NAMES
    worst = {"rouge": max(map(rel_err, arrays["rouge"].tolist(), want_arrays["rouge"])),
             "cider": max(map(rel_err, arrays["cider"].tolist(), want_arrays["cider"])),
             "corpus": max(rel_err(got[k], want[k]) for k in TC.NAMES)}
    print(f"caption scores N={n} vocab={vocab}: worst relative error {worst}; {got}")
    assert max(worst.values()) <= 1e-11, worst
    if n == 1:
        assert got["CIDEr"] == 0.0                           # log N = 0: every weight is 0
    if n > 1:                                                # the corpus exercises what it promises
        lengths = list(map(len, refs[0]))
        assert arrays["stats"][0, :2].tolist() == [4, 3] and lengths[:2] == [5, 3] and 4 not in lengths      # the tie goes to the shorter
        assert arrays["stats"][-1, 1].item() == 0 and arrays["rouge"][-1].item() == 0.0 and arrays["cider"][-1].item() == 0.0
    if n >= 7:
        assert {0, 128} <= set(arrays["stats"][:, 0].tolist()) and got["CIDEr"] > 0.0 and got["ROUGE_L"] > 0.0


def test_two_calls_give_identical_bits(dev):
    from multimodal import ops
    _c, _w, (got, arrays), t = _case(dev, 65, 5)
    again, arrays2 = ops.caption_scores(*t, 5)
    assert again == got
    for k in ("stats", "rouge", "cider"):
        assert torch.equal(arrays[k].view(torch.int64), arrays2[k].view(torch.int64)), k
    assert all(torch.equal(a, b) and torch.equal(c, d) for (a, c), (b, d) in zip(arrays["df"], arrays2["df"]))


def test_refusals(dev):
    from multimodal import _hip as H
    from multimodal import ops
    _c, _w, _g, (hyp, hyp_len, ref, ref_len, ref_off) = _case(dev, 7, 300)
    with pytest.raises(H.CvclError, match="non-contiguous"):
        ops.caption_scores(hyp.t().contiguous().t(), hyp_len, ref, ref_len, ref_off, 300)
    with pytest.raises(H.CvclError, match="non-contiguous"):
        ops.caption_scores(hyp, hyp_len, torch.cat([ref, ref], 1)[:, :ref.shape[1]], ref_len, ref_off, 300)
    for i in range(5):
        args = [hyp, hyp_len, ref, ref_len, ref_off]
        args[i] = args[i].cpu()
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            ops.caption_scores(*args, 300)
    with pytest.raises(H.CvclError, match="expected dtype"):
        ops.caption_scores(hyp.int(), hyp_len, ref, ref_len, ref_off, 300)
    with pytest.raises(ValueError, match=r"token ids outside \[0, 200\)"):
        ops.caption_scores(hyp, hyp_len, ref, ref_len, ref_off, 200)
    with pytest.raises(H.CvclError, match="vocab_size 32769"):
        ops.caption_scores(hyp, hyp_len, ref, ref_len, ref_off, 32769)


def test_evaluate_on_strings(dev):
    """A single string per example and a list per example; exactly the reference's names of the three scores; over a limit raises."""
    from multimodal import _hip as H
    from multimodal.textgen_eval import evaluate
    refs = [["the cat", "a dog"], ["a cat sat", "a cat sat down here", "sat"]]
    hyps = ["the the the", "a cat sat down"]
    got = evaluate(refs, hyps)
    want = TC.evaluate(refs, hyps)
    assert set(got) == set(TC.NAMES) == {"BLEU_1", "BLEU_2", "BLEU_3", "BLEU_4", "ROUGE_L", "CIDEr"}
    assert max(rel_err(got[k], want[k]) for k in TC.NAMES) <= 1e-11 and abs(got["CIDEr"] - 2.69957) < 1e-5
    single = evaluate(["a b d c", " a  cat "], ["a b c d", ""], keys=["x", "y"])
    want = TC.evaluate(["a b d c", "a cat"], ["a b c d", ""])
    assert set(single) == set(TC.NAMES) and max(rel_err(single[k], want[k]) for k in TC.NAMES) <= 1e-11
    assert evaluate(["a b d c"], ["a b c d"])["ROUGE_L"] == 0.75
    long = " ".join(f"w{i}" for i in range(129))
    with pytest.raises(H.CvclError, match="Lh 129 outside 1..128 tokens per sentence"):
        evaluate(["a"], [long])
    with pytest.raises(H.CvclError, match="Lr 129 outside 1..128 tokens per sentence"):
        evaluate([long], ["a"])
    with pytest.raises(H.CvclError, match=r"example 1 has 33 references \(outside 1..32\)"):
        evaluate([["a"], ["a"] * 33], ["a", "a"])
    with pytest.raises(H.CvclError, match="example 0 has 0 references"):
        evaluate([[], ["a"]], ["a", "a"])


def _caption_lm(dev, V, E, bias):
    import gen_golden_captioning as G
    from multimodal.multimodal import LanguageModel, TextEncoder
    vocab = {"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, **{f"w{i}": i for i in range(4, V)}}
    args = argparse.Namespace(text_encoder="lstm", embedding_type="flat", embedding_dim=E, crange=1, dropout_i=0.0, dropout_o=0.0,
                              pos_embed_type="no_pos_embed", captioning=True, attention=False, attention_gate=False, tie=True,
                              bias=True)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(vocab, 2048, args)
        lm = LanguageModel(te, args)
    G.fill_text_encoder(te)
    with torch.no_grad():
        lm.output_layer.bias.copy_(bias)
    return te.to(dev).eval(), lm.to(dev).eval()


def _lit_stub(dev, lm, encode):
    from multimodal.multimodal_lit import MultiModalLitModel
    lit = object.__new__(MultiModalLitModel)
    torch.nn.Module.__init__(lit)
    logged = {}
    lit.__dict__.update(lambda_mm=0.0, lambda_lm=1.0, optimize_unused=True, eval_textgen=True, beam_width=3, decode_length=25,
                        length_penalty_alpha=0.0, text_encoder=lm.text_encoder, training=False)
    lit.language_model = lm
    lit.model = types.SimpleNamespace(encode_image=encode, global_negatives=True)
    lit.log = lambda name, value, *a, **k: logged.__setitem__(name, value)
    return lit, logged


def test_epoch_end_logs_the_scores(dev):
    """calculate_joint_loss(eval_textgen=True) on two batches, then joint_loss_epoch_end: val_BLEU_1..4, val_ROUGE_L and val_CIDEr
    are logged and equal the restatement on the raw_y and gen_text the steps produced.  The references are made from a first
    decoding of the same images (its captions, shifted and cut), so that n-grams of every order match."""
    import gen_golden_captioning as G
    torch.manual_seed(4)
    _te, lm = _caption_lm(dev, 50, 32, G.output_bias(1.0))
    proj = torch.randn(3, 32, device=dev)
    encode = lambda x: (x.reshape(x.shape[0], -1)[:, :3] @ proj, None)       # a fixed "encoder": images -> flat features
    lit, logged = _lit_stub(dev, lm, encode)
    B = 6
    yb = torch.tensor([[2, 5, 6, 3]] * B, device=dev)
    ylb = torch.full((B,), 4, device=dev)
    outs = []
    with torch.no_grad():
        for _batch in range(2):
            xb = torch.randn(B, 3, 8, 8, device=dev)
            seq, _ = lm.beam_search_decode(B, 3, 25, 0.0, image_features=encode(xb)[0])
            first = [lit._ids_to_sentence(s) for s in seq[:, 0].tolist()]
            raw_y = [[first[i], " ".join(first[(i + 1) % B].split()[1:]) + " w7"] if i % 2 else first[i] + " w5" for i in range(B)]
            outs.append(lit.calculate_joint_loss((xb, yb, ylb, raw_y), "val", lambda *a, **k: None, eval_textgen=True))
            assert outs[-1]["raw_y"] == raw_y and outs[-1]["gen_text"] == first
    with contextlib.redirect_stdout(io.StringIO()) as so:
        lit.joint_loss_epoch_end(outs, "val", lit.log, eval_textgen=True)
    assert "hypothesis:" in so.getvalue()
    want = TC.evaluate([r for o in outs for r in o["raw_y"]], [h for o in outs for h in o["gen_text"]])
    assert {f"val_{k}" for k in TC.NAMES} <= set(logged)
    worst = max(rel_err(logged[f"val_{k}"], want[k]) for k in TC.NAMES)
    print(f"epoch end: {({k: logged[f'val_{k}'] for k in TC.NAMES})}; worst relative error {worst}")
    assert worst <= 1e-11
    assert want["BLEU_1"] > 0.1 and want["ROUGE_L"] > 0.1                                      # the scores are not trivial


def test_bench_tool_runs_and_reports_median_min_max(capsys):
    """tools/bench_textgen_scores.py at a toy size: one JSON line, every timed entry with its minimum and maximum (K, min_K, max_K),
    and the device scores within the bound of the restatement's."""
    import json

    import bench_textgen_scores
    bench_textgen_scores.main(["--examples", "40", "--host-repeats", "2", "--repeats", "2", "--window-ms", "2"])
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    for side in ("evaluate", "caption_scores", "host_restatement"):
        assert 0 < res[side]["min_ms"] <= res[side]["ms"] <= res[side]["max_ms"], side
    assert res["shape"]["examples"] == 40 and res["shape"]["references"] == 200 and set(res["scores"]) == set(TC.NAMES)
    assert res["max_rel_diff"] <= 1e-11 and res["ids_equal_strings_max_rel_diff"] == 0.0 and res["host_over_evaluate"] > 0
