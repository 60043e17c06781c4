"""CPU: the packed-key restatement of tests/ngram_common.py against the reference's own n-gram model, recorded in
tests/golden/ngram.npz by tools/gen_golden_ngram.py: the counts equal, the float32 token losses BIT-equal, the tokenwise=False
scalar equal, on the five cases at both alphas.  Every branch of the back-off chain that a case's N and vocabulary allow must be
hit by its evaluation corpus -- a condition on the inputs, so that no case passes on one branch only."""
import numpy as np
import pytest
import torch

import ngram_common as NC
from conftest import load_golden


@pytest.fixture(scope="module")
def z():
    return load_golden("ngram")


def golden_counts(z, case):
    """The archive's counts of a case in the reference's ``_count`` shape."""
    name = NC.case_name(case)
    out = []
    for n in range(case[0]):
        ctx, word, cnt, total = (z[f"{name}.count{n}.{f}"].numpy() for f in ("ctx", "word", "cnt", "total"))
        table = {}
        for c, w, k, t in zip(ctx.tolist(), word.tolist(), cnt.tolist(), total.tolist()):
            entry = table.setdefault(tuple(c), [t, {}])
            assert entry[0] == t
            entry[1][w] = k
        assert all(e[0] == sum(e[1].values()) for e in table.values())          # total += 1 goes with every next[w] += 1
        out.append(table)
    return out


def test_archive_holds_the_case_table(z):
    assert [tuple(c) for c in z["cases"].tolist()] == list(NC.CASES) and tuple(z["alphas"].tolist()) == NC.ALPHAS


@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_name)
def test_restatement_equals_the_reference(z, case):
    N, V, B, L = case
    name = NC.case_name(case)
    (ty, tl), (ey, el) = NC.case_data(case)
    for mine, stored in ((ty, "train_y"), (tl, "train_len"), (ey, "eval_y"), (el, "eval_len")):
        assert np.array_equal(mine, z[f"{name}.{stored}"].numpy())               # the generator gives the recorded corpora
    assert min(tl.min(), el.min()) >= 1 and max(tl.max(), el.max()) <= L and ty.shape == ey.shape == (B, L)
    tables = NC.count_tables(ty, tl, N, V)
    assert NC.to_counts(tables, V) == golden_counts(z, case)
    model = NC.Model(N, V, tables)
    for alpha in NC.ALPHAS:
        loss, loss64, hist = model.ce_loss(ey, el, alpha)
        want = z[f"{name}.loss_a{alpha}"].numpy()
        assert loss.dtype == want.dtype == np.float32 and np.array_equal(loss.view(np.int32), want.view(np.int32))
        mean = torch.from_numpy(loss).sum() / NC.n_tokens(el, L)                 # the reference's float32 sum over its count
        assert np.float32(mean.item()) == z[f"{name}.mean_a{alpha}"].numpy()
        assert sum(hist.values()) == NC.n_tokens(el, L)
        missing = [b for b in NC.branches_allowed(case) if not hist.get(b)]
        assert not missing, (missing, hist)


def test_several_updates_equal_one():
    """Runs no product code: it pins the merge path of the restatement's count_tables (its ``tables`` argument), which the GPU
    tests use as the oracle for updates in batches.  Not coverage of the feature."""
    case = NC.CASES[2]
    N, V, _B, _L = case
    (ty, tl), _eval = NC.case_data(case)
    tables = None
    for lo, hi in ((0, 3), (3, 4), (4, 40)):
        tables = NC.count_tables(ty[lo:hi], tl[lo:hi], N, V, tables)
    whole = NC.count_tables(ty, tl, N, V)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(tables, whole))


def test_probabilities_agree_with_the_loss():
    """Runs no product code: it pins the restatement's ``probs`` (the vectorised walk over all candidates), which the GPU tests
    use as the oracle for cvcl_ngram_probs, to its scalar walk: at the word that is there, exp(-loss).  Not coverage of the
    feature."""
    case = NC.CASES[2]
    N, V, _B, _L = case
    (ty, tl), (ey, el) = NC.case_data(case)
    model = NC.Model(N, V, NC.count_tables(ty, tl, N, V))
    probs = model.probs(ey, el, 0.1)
    _l32, loss64, _h = model.ce_loss(ey, el, 0.1)
    for b in range(len(ey)):
        n = int(el[b])
        for i in range(1, n):
            assert probs[b, i - 1, ey[b, i]] == np.exp(-loss64[b, i - 1]) or \
                abs(probs[b, i - 1, ey[b, i]] - np.exp(-loss64[b, i - 1])) <= 2e-16 * probs[b, i - 1, ey[b, i]]
        assert np.all(probs[b, max(n - 1, 0):] == 0)
