"""The yardstick of the caption-score tests: a plain-Python float64 restatement of the three pycocoevalcap scorers the reference's
multimodal/textgen_eval.py calls that are pure n-gram arithmetic -- BLEU-1..4 (corpus level, option "closest"), ROUGE-L (beta 1.2)
and CIDEr (n = 1..4, sigma = 6, log_N = log(float(N))) -- with default arguments and no PTB tokenizer, on dicts of token tuples and a
classic LCS table.  A sentence is a list of hashable tokens (words or ids); ``tokens`` turns a string into one with ``split()``.
The package itself is not installed where these tests run, so parity with it is not pinned: this file states its definitions.

Also the seeded corpus of the GPU tests and of tools/bench_textgen_scores.py."""
import math
import random

ORDERS = 4
NAMES = ("BLEU_1", "BLEU_2", "BLEU_3", "BLEU_4", "ROUGE_L", "CIDEr")


def tokens(sentence):
    return sentence.split()


def ngram_counts(s, n):
    """{n-gram tuple: occurrences}, in order of first occurrence"""
    out = {}
    for i in range(len(s) - n + 1):
        g = tuple(s[i:i + n])
        out[g] = out.get(g, 0) + 1
    return out


# ---- BLEU (bleu_scorer.py: cook_refs, cook_test, compute_score) ----
def bleu_stats(hyp, refs):
    """-> [testlen, reflen, guess_1..4, correct_1..4] of one example"""
    testlen = len(hyp)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    guess, correct = [], []
    for n in range(1, ORDERS + 1):
        ref_counts = [ngram_counts(r, n) for r in refs]
        guess.append(max(0, testlen - n + 1))
        correct.append(sum(min(c, max(rc.get(g, 0) for rc in ref_counts)) for g, c in ngram_counts(hyp, n).items()))
    return [testlen, reflen] + guess + correct


def bleu_from_totals(totals):
    testlen, reflen, guess, correct = totals[0], totals[1], totals[2:6], totals[6:10]
    tiny, small = 1e-15, 1e-9
    ratio = (testlen + tiny) / (reflen + small)
    out, b = [], 1.0
    for k in range(ORDERS):
        b *= (correct[k] + tiny) / (guess[k] + small)
        score = b ** (1.0 / (k + 1))
        if ratio < 1:
            score *= math.exp(1 - 1 / ratio)
        out.append(score)
    return out


# ---- ROUGE-L (rouge.py: my_lcs, calc_score) ----
def lcs(a, b):
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def rouge_l(hyp, refs, beta=1.2):
    prec = max(lcs(hyp, r) / len(hyp) if hyp else 0.0 for r in refs)
    rec = max(lcs(hyp, r) / len(r) if r else 0.0 for r in refs)
    if prec != 0 and rec != 0:
        return ((1 + beta ** 2) * prec * rec) / (rec + beta ** 2 * prec)
    return 0.0


# ---- CIDEr (cider_scorer.py: compute_doc_freq, counts2vec, sim, compute_cider) ----
def document_frequency(list_of_refs):
    """-> per order n = 1..4 {n-gram: the number of examples whose references hold it}"""
    df = [{} for _ in range(ORDERS)]
    for refs in list_of_refs:
        for n in range(1, ORDERS + 1):
            for g in {g for r in refs for g in ngram_counts(r, n)}:
                df[n - 1][g] = df[n - 1].get(g, 0) + 1
    return df


def _vector(s, df, log_n):
    vec, norm = [], []
    for n in range(1, ORDERS + 1):
        v = {g: float(tf) * (log_n - math.log(max(1.0, df[n - 1].get(g, 0)))) for g, tf in ngram_counts(s, n).items()}
        vec.append(v)
        norm.append(math.sqrt(sum(x * x for x in v.values())))
    return vec, norm, max(0, len(s) - 1)                   # "length": the number of bigram occurrences


def cider(hyps, list_of_refs, sigma=6.0):
    """-> (per-example scores, the document frequencies)"""
    df = document_frequency(list_of_refs)
    log_n = math.log(float(len(hyps)))
    out = []
    for hyp, refs in zip(hyps, list_of_refs):
        vec_h, norm_h, len_h = _vector(hyp, df, log_n)
        score = [0.0] * ORDERS
        for ref in refs:
            vec_r, norm_r, len_r = _vector(ref, df, log_n)
            delta = float(len_h - len_r)
            for n in range(ORDERS):
                val = 0.0
                for g, h in vec_h[n].items():
                    r = vec_r[n].get(g, 0.0)
                    val += min(h, r) * r
                if norm_h[n] != 0 and norm_r[n] != 0:
                    val /= norm_h[n] * norm_r[n]
                score[n] += val * math.exp(-(delta ** 2) / (2 * sigma ** 2))
        out.append((((score[0] + score[1]) + score[2]) + score[3]) / ORDERS / len(refs) * 10.0)
    return out, df


def score_corpus(hyps, list_of_refs):
    """hyps[i]: a token list; list_of_refs[i]: its reference token lists -> (scores {name: float}, per-example arrays
    {"stats": [[10 ints]], "rouge": [float], "cider": [float], "df": [{n-gram: count}] per order})"""
    stats = [bleu_stats(h, r) for h, r in zip(hyps, list_of_refs)]
    rouge = [rouge_l(h, r) for h, r in zip(hyps, list_of_refs)]
    cid, df = cider(hyps, list_of_refs)
    bleu = bleu_from_totals([sum(col) for col in zip(*stats)])
    scores = dict(zip(NAMES, bleu + [sum(rouge) / len(rouge), sum(cid) / len(cid)]))
    return scores, {"stats": stats, "rouge": rouge, "cider": cid, "df": df}


def evaluate(list_of_references, hypotheses):
    """multimodal.textgen_eval.evaluate on strings: a reference entry is one string or a list of strings"""
    refs = [[tokens(s) for s in (r if isinstance(r, (list, tuple)) else [r])] for r in list_of_references]
    return score_corpus([tokens(h) for h in hypotheses], refs)[0]


def tensors(hyps, list_of_refs, device):
    """id sentences -> ops.caption_scores' (hyp, hyp_len, ref, ref_len, ref_off): int64, rows zero padded to the widest (at least 1)"""
    import torch

    def rows(sentences):
        width = max(1, max(map(len, sentences)))
        ids = torch.tensor([s + [0] * (width - len(s)) for s in sentences], dtype=torch.int64)
        return ids.to(device), torch.tensor([len(s) for s in sentences], dtype=torch.int64).to(device)

    offsets = [0]
    for r in list_of_refs:
        offsets.append(offsets[-1] + len(r))
    return (*rows(hyps), *rows([s for r in list_of_refs for s in r]), torch.tensor(offsets, dtype=torch.int64).to(device))


def unpack_df(keys, counts, n, vocab):
    """a device table of order n (packed keys, counts) -> {n-gram tuple: count}"""
    bits = max(1, (vocab - 1).bit_length())
    return {tuple((k >> ((n - 1 - j) * bits)) & ((1 << bits) - 1) for j in range(n)): c for k, c in zip(keys.tolist(), counts.tolist())}


# ---- seeded corpora ----
HYP_LENGTHS = (0, 1, 2, 3, 4, 25, 128)


def corpus(seed, n, vocab, hyp_lengths=HYP_LENGTHS, max_refs=5, ref_tokens=None):
    """-> (hyps, list_of_refs) of ids in [0, vocab).  Hypothesis lengths go through ``hyp_lengths`` in turn, example 0 at 4 tokens;
    an example has 1 .. ``max_refs`` references.  A reference is a noisy copy of the hypothesis (so n-grams of every order match),
    a slice of another example's hypothesis, random ids, or empty.  Example 0 has references of 3 and 5 tokens first (a ``reflen``
    tie), and with n > 1 the LAST example has nothing but empty references.  ``ref_tokens``: every sentence has about that many
    tokens and every example ``max_refs`` references instead (the bench corpus)."""
    rng = random.Random(seed)
    word = lambda: rng.randrange(vocab)                                        # noqa: E731
    if ref_tokens:
        hyps = [[word() for _ in range(max(1, ref_tokens + rng.randint(-3, 3)))] for _ in range(n)]
    else:
        start = hyp_lengths.index(4)                                           # lengths in turn, example 0 at 4 tokens
        hyps = [[word() for _ in range(hyp_lengths[(start + i) % len(hyp_lengths)])] for i in range(n)]

    def noisy(h, length):
        out = [t if rng.random() < 0.7 else word() for t in h]
        while len(out) < length:
            out.insert(rng.randrange(len(out) + 1), word())
        while len(out) > length:
            del out[rng.randrange(len(out))]
        return out

    list_of_refs = []
    for i, h in enumerate(hyps):
        count = max_refs if ref_tokens else rng.randint(1, max_refs)
        refs = []
        for _ in range(count):
            kind = rng.random()
            length = max(1, ref_tokens + rng.randint(-3, 3)) if ref_tokens else min(128, max(0, len(h) + rng.randint(-3, 3)))
            if kind < 0.6:
                refs.append(noisy(h, length))
            elif kind < 0.8:
                other = hyps[rng.randrange(n)]
                refs.append(other[:length])
            elif kind < 0.93 or ref_tokens:
                refs.append([word() for _ in range(length)])
            else:
                refs.append([])
        if i == 0 and not ref_tokens:
            refs = [noisy(h, 5), noisy(h, 3)] + [r for r in refs[2:] if len(r) != 4]
        if i == n - 1 and n > 1 and not ref_tokens:
            refs = [[] for _ in refs]
        list_of_refs.append(refs)
    return hyps, list_of_refs
