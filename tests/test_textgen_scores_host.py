"""CPU: the float64 restatement of the caption scores (tests/textgen_scores_common.py), the yardstick of the GPU tests, on two
corpora worked by hand; ops.bleu_from_totals, the host lines behind the device statistics, against the restatement's."""
import math

import pytest

import textgen_scores_common as TC

TINY, SMALL = 1e-15, 1e-9


def close(got, want):
    return got == pytest.approx(want, rel=1e-12, abs=1e-15)


def test_worked_case_one_example():
    """Hypothesis `a b c d`, one reference `a b d c`: the unigrams all match, of the bigrams only `a b`; LCS = 3 (`a b c` or
    `a b d`), p = r = 3/4, and ROUGE_L = (1 + b^2) p r / (r + b^2 p) = p when p = r.  N = 1: log N = 0, every CIDEr weight is 0.
    testlen = reflen = 4, yet ratio = (4 + tiny) / (4 + small) is below 1 by 2.5e-10, so the brevity penalty exp(1 - 1 / ratio) =
    exp(-2.5e-10) applies, as it does in the package: BLEU_2 is sqrt((4 + tiny) / (4 + small) (1 + tiny) / (3 + small)) times that."""
    scores, arrays = TC.score_corpus([TC.tokens("a b c d")], [[TC.tokens("a b d c")]])
    assert arrays["stats"] == [[4, 4, 4, 3, 2, 1, 4, 1, 0, 0]]
    assert TC.lcs(TC.tokens("a b c d"), TC.tokens("a b d c")) == 3
    assert close(scores["ROUGE_L"], 0.75)
    penalty = math.exp(1 - (4 + SMALL) / (4 + TINY))
    assert close(scores["BLEU_1"], (4 + TINY) / (4 + SMALL) * penalty)
    bleu_2 = math.sqrt((4 + TINY) / (4 + SMALL) * (1 + TINY) / (3 + SMALL))
    assert close(scores["BLEU_2"], bleu_2 * penalty) and abs(scores["BLEU_2"] - bleu_2) < 1e-9
    b3 = (4 + TINY) / (4 + SMALL) * (1 + TINY) / (3 + SMALL) * TINY / (2 + SMALL)
    assert close(scores["BLEU_3"], b3 ** (1 / 3) * penalty) and close(scores["BLEU_4"], (b3 * TINY / (1 + SMALL)) ** 0.25 * penalty)
    assert scores["CIDEr"] == 0.0 and arrays["cider"] == [0.0]
    assert TC.evaluate(["a b d c"], ["a b c d"]) == scores == TC.evaluate([["a b d c"]], ["a b c d"])
    assert tuple(scores) == TC.NAMES


REFS = [["the cat", "a dog"], ["a cat sat", "a cat sat down here", "sat"]]
HYPS = ["the the the", "a cat sat down"]


def test_worked_case_two_examples():
    """Example 1: `the the the` against `the cat`, `a dog`.  Example 2: `a cat sat down` against `a cat sat`, `a cat sat down
    here`, `sat`.

    BLEU.  Example 1: testlen 3, both references have 2 tokens, reflen 2; guess = [3, 2, 1, 0]; `the` occurs 3 times but once in
    the best reference, so it is clipped to 1: correct = [1, 0, 0, 0].  Example 2: testlen 4, reference lengths 3, 5, 1: 3 and 5
    are equally close and the tie goes to the shorter, reflen 3; every n-gram is in the second reference: guess = correct =
    [4, 3, 2, 1].  Totals: testlen 7, reflen 5 (no brevity penalty), guess [7, 5, 3, 1], correct [5, 3, 2, 1].

    ROUGE-L.  Example 1: LCS 1 with `the cat` (p 1/3, r 1/2), 0 with `a dog`: 2.44 (1/6) / (1/2 + 1.44/3).  Example 2: LCS 3, 4, 1:
    p = max(3/4, 4/4, 1/4) = 1 from the second reference, r = max(3/3, 4/5, 1/1) = 1 from the others: 1.

    CIDEr.  N = 2, L = log 2.  Document frequencies: `cat` and `a` are in both examples' references (weight L - log 2 = 0), every
    other n-gram of the references in one (weight L); `the the`, `the the the` are in none (weight L - log 1 = L).  Every vector
    entry is a multiple of L, so L cancels in every normalised product.  g1 = exp(-1/72), g3 = exp(-9/72).
    Example 1: h_1 = {the: 3L}, |h_1| = 3L, 2 bigrams.  `the cat`: r_1 = {the: L, cat: 0}, |r_1| = L, 1 bigram:
    min(3L, L) L / (3L L) = 1/3, times g1; its bigram and the hypothesis' do not meet; `a dog` shares nothing.
    score = 10 (1/3 g1 / 4) / 2.
    Example 2: h_1 = {a: 0, cat: 0, sat: L, down: L}, |h_1| = L sqrt 2; three bigrams at L, |h_2| = L sqrt 3; two trigrams,
    |h_3| = L sqrt 2; one 4-gram, |h_4| = L; 3 bigrams.
      `a cat sat` (norms L, L sqrt 2, L, 0; 2 bigrams, g1): 1/sqrt 2, 2/sqrt 6, 1/sqrt 2, 0.
      `a cat sat down here` (norms L sqrt 3, 2L, L sqrt 3, L sqrt 2; 4 bigrams, g1): 2/sqrt 6, 3/(2 sqrt 3), 2/sqrt 6, 1/sqrt 2.
      `sat` (norm L; 0 bigrams, g3): 1/sqrt 2, 0, 0, 0.
    score = 10 ((g1 (1/sqrt 2 + 2/sqrt 6) + g3/sqrt 2) + g1 (2/sqrt 6 + sqrt 3/2) + g1 (1/sqrt 2 + 2/sqrt 6) + g1/sqrt 2) / 4 / 3.
    CIDEr = (0.41092 + 4.98822) / 2 = 2.69957."""
    hyps = [TC.tokens(h) for h in HYPS]
    refs = [[TC.tokens(s) for s in r] for r in REFS]
    scores, arrays = TC.score_corpus(hyps, refs)
    assert arrays["stats"] == [[3, 2, 3, 2, 1, 0, 1, 0, 0, 0], [4, 3, 4, 3, 2, 1, 4, 3, 2, 1]]
    b, want = 1.0, []
    for k, (c, g) in enumerate(zip([5, 3, 2, 1], [7, 5, 3, 1])):
        b *= (c + TINY) / (g + SMALL)
        want.append(b ** (1 / (k + 1)))
    assert all(close(scores[f"BLEU_{k + 1}"], w) for k, w in enumerate(want))
    assert abs(scores["BLEU_1"] - 5 / 7) < 1e-9 and abs(scores["BLEU_4"] - (2 / 7) ** 0.25) < 1e-9      # tiny and small aside
    assert close(arrays["rouge"][0], 2.44 * (1 / 6) / (1 / 2 + 1.44 / 3)) and close(arrays["rouge"][1], 1.0)
    assert close(scores["ROUGE_L"], (2.44 / 6 / (0.5 + 0.48) + 1.0) / 2)
    assert [sorted(d.items()) for d in arrays["df"][:1]] == [sorted({("the",): 1, ("cat",): 2, ("a",): 2, ("dog",): 1, ("sat",): 1,
                                                                      ("down",): 1, ("here",): 1}.items())]
    assert [len(d) for d in arrays["df"]] == [7, 6, 3, 2] and all(v == 1 for d in arrays["df"][1:] for v in d.values())
    g1, g3, s2, s3, s6 = math.exp(-1 / 72), math.exp(-9 / 72), math.sqrt(2), math.sqrt(3), math.sqrt(6)
    one = 10 * (g1 / 3 / 4) / 2
    two = 10 * ((g1 * (1 / s2 + 2 / s6) + g3 / s2) + g1 * (2 / s6 + s3 / 2) + g1 * (1 / s2 + 2 / s6) + g1 / s2) / 4 / 3
    assert close(arrays["cider"][0], one) and close(arrays["cider"][1], two)
    assert close(scores["CIDEr"], (one + two) / 2) and abs(scores["CIDEr"] - 2.69957) < 1e-5 and abs(one - 0.41092) < 1e-5
    assert TC.evaluate(REFS, HYPS) == scores


def test_tokens_are_split_on_any_whitespace():
    assert TC.tokens("  a  b ") == ["a", "b"] and TC.tokens("") == []
    assert TC.evaluate(["a b"], [""]) == dict(zip(TC.NAMES, [0.0] * 6))       # the empty hypothesis: brevity penalty exp(-2e15)
    assert TC.evaluate([" a  b"], ["a b "]) == TC.evaluate(["a b"], ["a b"])


def test_seeded_corpus_covers_what_the_gpu_tests_need():
    lengths, ties, empties, counts = set(), 0, 0, set()
    for n in (1, 2, 7, 65):
        for vocab in (5, 300):
            hyps, refs = TC.corpus(n, n, vocab)
            assert len(hyps) == len(refs) == n and all(1 <= len(r) <= 5 for r in refs)
            assert all(0 <= t < vocab for s in hyps + [s for r in refs for s in r] for t in s)
            assert all(len(s) <= 128 for r in refs for s in r)
            lengths |= set(map(len, hyps))
            counts |= set(map(len, refs))
            for h, r in zip(hyps, refs):
                near = sorted((abs(len(s) - len(h)), len(s)) for s in r)
                ties += len(near) > 1 and near[0][0] == near[1][0] and near[0][1] != near[1][1]
                empties += all(not s for s in r)
            assert TC.corpus(n, n, vocab) == (hyps, refs)                          # seeded
    assert lengths == set(TC.HYP_LENGTHS) and ties >= 8 and empties >= 6 and counts == {1, 2, 3, 4, 5}


def test_host_bleu_lines_equal_the_restatement():
    from multimodal import ops
    for totals in ([7, 5, 7, 5, 3, 1, 5, 3, 2, 1], [4, 9, 4, 3, 2, 1, 4, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 3, 2, 1, 0, 3, 2, 1, 0]):
        assert ops.bleu_from_totals(totals) == TC.bleu_from_totals(totals)
