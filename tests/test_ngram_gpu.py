"""GPU: the n-gram baseline (csrc/ngram.hip, ngram.NGramModel, its path through analysis_tools.processing and word_statistics.py)
against the reference's recorded results (tests/golden/ngram.npz) and, off the archive, against the restatement of
tests/ngram_common.py, which tests/test_ngram_fixture.py pins to the reference bit for bit.

Bounds.  Counts are integers: equal.  A token loss is a float64 sum of a few logs rounded once to float32; the device's sum is off
by a few float64 steps (its log is not the host's), so its rounding can differ from the reference's by at most ONE float32 step:
every element within 1 ulp.  The same for a probability against exp of the restatement's float64 log-probability.
-log(probs) against the loss: 1 ulp on p is 2^-23 relative, i.e. 2^-23 absolute on its log, plus 1 ulp on the loss, 2^-23 max(1, loss)
-> 2^-22 max(1, loss).  tokenwise=False: a float32 sum of B L non-negative terms, B L 2^-24 relative."""
import csv
import math

import numpy as np
import pytest
import torch

import ngram_common as NC
from test_ngram_fixture import golden_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    from conftest import load_golden
    return load_golden("ngram")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _trained(case, dev, data=None):
    from ngram import NGramModel
    (ty, tl), _e = data or NC.case_data(case)
    model = NGramModel(case[0], case[1], device=dev)
    model.update(_t(ty), _t(tl))
    return model


def _check_loss(got, want32, y_len, L, what):
    """got [B, L - 1] device f32 against the float32 reference values: <= 1 ulp, exact zeros outside; prints the bit-equal share."""
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want32.shape
    d = NC.ulp_distance(got, want32)
    inside = np.arange(1, L)[None, :] < np.minimum(y_len, L)[:, None]
    share = float((d[inside] == 0).mean()) if inside.any() else 1.0
    print(f"[ngram {what}] {int(inside.sum())} tokens: bit-equal {share:.4f}, worst {int(d.max()) if d.size else 0} ulp")
    assert np.all(got[~inside] == 0) and np.all(np.isfinite(got))
    assert d.size == 0 or d.max() <= 1, (what, int(d.max()))
    return share


# ----------------------------------------------------------------------------- counts
@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_name)
def test_counts_equal_the_reference(z, dev, case):
    assert _trained(case, dev).to_counts() == golden_counts(z, case)


def test_updates_in_batches_and_after_scoring(dev):
    from ngram import NGramModel
    case = NC.CASES[2]
    N, V, B, L = case
    (ty, tl), (ey, el) = NC.case_data(case)
    whole = _trained(case, dev)
    parts = NGramModel(N, V, device=dev)
    for lo, hi in ((0, 3), (3, 4), (4, B)):
        parts.update(_t(ty[lo:hi]), _t(tl[lo:hi]))
    assert parts.to_counts() == whole.to_counts()
    # scoring, then update, then scoring again: the new counts are used
    first = whole.calculate_ce_loss(_t(ey), _t(el))
    whole.update(_t(ey), _t(el))
    tables = NC.count_tables(np.concatenate([ty, ey]), np.concatenate([tl, el]), N, V)
    assert whole.to_counts() == NC.to_counts(tables, V)
    second = whole.calculate_ce_loss(_t(ey), _t(el))
    want, _l64, _h = NC.Model(N, V, tables).ce_loss(ey, el, 0.1)
    _check_loss(second, want, el, L, "after a second update")
    assert not torch.equal(first, second)
    # an update after to_counts() of a merged table (old keys and counts + new keys)
    parts.update(_t(ey), _t(el))
    assert parts.to_counts() == whole.to_counts()


# ----------------------------------------------------------------------------- loss
@pytest.mark.parametrize("alpha", NC.ALPHAS)
@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_name)
def test_loss_within_one_ulp_of_the_reference(z, dev, case, alpha):
    from multimodal import ops
    N, V, B, L = case
    name = NC.case_name(case)
    _train, (ey, el) = NC.case_data(case)
    model = _trained(case, dev)
    want = z[f"{name}.loss_a{alpha}"].numpy()
    got = model.calculate_ce_loss(_t(ey), _t(el), alpha=alpha)
    assert got.device == dev or got.device.type == "cuda"
    _check_loss(got, want, el, L, f"{name} alpha {alpha}")
    # the kernel writes every element: zeros outside the utterances in a buffer that held NaN
    out = torch.full((B, L - 1), float("nan"), device=dev)
    loss, bad = ops.ngram_ce_loss(model._rebuild(), N, V, math.log(alpha), math.log(1 - alpha), _t(ey).to(dev), _t(el).to(dev), out=out)
    assert loss is out and int(bad.item()) == 0 and torch.equal(out, got)        # and a second call gives the same bits
    # tokenwise=False: the float32 mean against the float64 sum of the golden token losses
    n_tok = NC.n_tokens(el, L)
    mean = model.calculate_ce_loss(_t(ey), _t(el), alpha=alpha, tokenwise=False)
    want_mean = float(want.astype(np.float64).sum()) / n_tok
    assert mean.dim() == 0 and abs(float(mean) - want_mean) <= B * L * 2.0 ** -24 * want_mean


# ----------------------------------------------------------------------------- edges
def test_short_utterances_clamped_lengths_and_empty_inputs(dev):
    from ngram import NGramModel
    N, V, L = 3, 30, 6
    (ty, tl), _e = NC.corpus(5, V, 20, L), None
    model = NGramModel(N, V, device=dev)
    model.update(_t(ty), _t(tl))
    rest = NC.Model(N, V, NC.count_tables(ty, tl, N, V))
    y = np.array([[1, 4, 5, 3, 7, 2], [1, 2, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 3, 3, 2, 9, 9], [1, 5, 2, 0, 0, 0]], dtype=np.int64)
    y_len = np.array([9, 2, 1, 0, 3], dtype=np.int64)                             # 9 > L: clamped; lengths 2, 1 and 0
    want, _l64, _h = rest.ce_loss(y, y_len, 0.1)
    _check_loss(model.calculate_ce_loss(_t(y), _t(y_len)), want, y_len, L, "short and clamped")
    before = model.to_counts()
    model.update(_t(y[2:4]), _t(y_len[2:4]))                                      # lengths 1 and 0 count nothing
    assert model.to_counts() == before
    model.update(_t(y[:1]), _t(y_len[:1]))                                        # a clamped length counts the whole row
    assert model.to_counts() == NC.to_counts(NC.count_tables(y[:1], y_len[:1], N, V, rest.grams), V)
    for shape in ((0, L), (4, 1), (0, 1)):
        yy, ll = torch.zeros(shape, dtype=torch.long), torch.ones(shape[0], dtype=torch.long)
        loss = model.calculate_ce_loss(yy, ll)
        assert tuple(loss.shape) == (shape[0], 0) and loss.dtype == torch.float32 and loss.device.type == "cuda"
        assert math.isnan(float(model.calculate_ce_loss(yy, ll, tokenwise=False)))                # 0 / 0, as the reference
        assert tuple(model.calculate_probs(yy, ll).shape) == (shape[0], shape[1] - 1, V)
        model.update(yy, ll)
    assert math.isnan(float(model.calculate_ce_loss(_t(y[2:4]), _t(y_len[2:4]), tokenwise=False)))
    empty = NGramModel(N, V, device=dev)
    empty.update(_t(y[2:4]), _t(y_len[2:4]))
    for fn in (empty.calculate_ce_loss, empty.calculate_probs):
        with pytest.raises(Exception, match="Even unigram is not applicable."):
            fn(_t(y), _t(y_len))
    assert empty.to_counts() == [{}, {}, {}]


def test_unseen_contexts_in_the_project_case():
    """The evaluation corpus of (3, 2350, 64, 25) holds contexts the training corpus never had (a condition on the inputs)."""
    case = NC.CASES[4]
    (ty, tl), (ey, el) = NC.case_data(case)
    ctxs = NC.context_tables(NC.count_tables(ty, tl, *case[:2]), case[1])
    seen = set(ctxs[2][0].tolist())
    bits = NC.key_bits(case[1])
    assert any(NC.pack(ey[b, i - 2:i], bits) not in seen for b in range(len(ey)) for i in range(2, int(el[b])))


@pytest.mark.parametrize("N,V,top", [(5, 2, None), (3, 65536, 65535), (5, 4096, 4095)], ids=["v2_n5", "v65536_n3", "v4096_n5_top_id"])
def test_key_widths(dev, N, V, top):
    """1-bit tokens; 48 key bits with the top id in use; case (5, 4096, 64, 12), 60 key bits, with an utterance of the top id
    appended to both of its splits."""
    rng = np.random.default_rng(V + N)
    B, L = 24, 12
    if V == 2:
        def draw():
            y = rng.integers(0, 2, (B, L)).astype(np.int64)
            y[:, 0] = 1
            return y, rng.integers(1, L + 1, B).astype(np.int64)
        (ty, tl), (ey, el) = draw(), draw()
    else:
        if (N, V) == NC.CASES[3][:2]:
            (ty, tl), (ey, el) = NC.case_data(NC.CASES[3])
        else:
            (ty, tl), (ey, el) = NC.corpus(N, V, B, L), NC.corpus(100 + N, V, B, L)
        extra = np.full((1, L), top, dtype=np.int64)
        ty, tl = np.concatenate([ty, extra]), np.concatenate([tl, [L]])
        ey, el = np.concatenate([ey, extra]), np.concatenate([el, [L - 1]])
    model = _trained((N, V), dev, ((ty, tl), None))
    tables = NC.count_tables(ty, tl, N, V)
    assert model.to_counts() == NC.to_counts(tables, V)
    want, _l64, hist = NC.Model(N, V, tables).ce_loss(ey, el, 0.1)
    assert hist.get(("order", N - 1))                                             # the widest keys are looked up and found
    _check_loss(model.calculate_ce_loss(_t(ey), _t(el)), want, el, ey.shape[1], f"V {V} N {N}")


def test_cpu_int32_and_strided_inputs_give_the_same_bits(dev):
    from ngram import NGramModel
    case = NC.CASES[2]
    N, V, B, L = case
    (ty, tl), (ey, el) = NC.case_data(case)
    plain = _trained(case, dev)
    want = plain.calculate_ce_loss(_t(ey).to(dev), _t(el).to(dev))
    wide = np.zeros((B, 2 * L), dtype=np.int64)
    wide[:, ::2] = ey
    for y, n in ((_t(ey), _t(el)), (_t(ey).int(), _t(el).int()), (_t(ey).to(dev).short(), _t(el).to(dev).to(torch.uint8)),
                 (_t(wide)[:, ::2], _t(el)), (_t(ey.T.copy()).to(dev).t(), _t(el))):
        got = plain.calculate_ce_loss(y, n)
        assert got.device.type == "cuda" and torch.equal(got, want)
    other = NGramModel(N, V, device=dev)
    other.update(_t(ty).int()[:, :], _t(tl).int())
    assert other.to_counts() == plain.to_counts()
    assert torch.equal(plain.calculate_probs(_t(ey).int(), _t(el)), plain.calculate_probs(_t(ey).to(dev), _t(el).to(dev)))


def test_bad_ids_raise_inside_the_lengths_only(dev):
    from ngram import NGramModel
    N, V, L = 3, 30, 6
    ty, tl = NC.corpus(5, V, 20, L)
    model = NGramModel(N, V, device=dev)
    model.update(_t(ty), _t(tl))
    counts = model.to_counts()
    for bad_id in (V, -1):
        y = np.array([[1, 4, 5, 2, 0, 0], [1, 3, 2, 0, 0, 0]], dtype=np.int64)
        y_len = np.array([4, 3], dtype=np.int64)
        y[1, 4] = bad_id                                                          # in the padding: nobody minds
        want = model.calculate_ce_loss(_t(y), _t(y_len))
        model.calculate_probs(_t(y), _t(y_len))
        y[0, 2] = bad_id
        for fn in (model.update, model.calculate_ce_loss, model.calculate_probs):
            with pytest.raises(ValueError, match=r"outside \[0, 30\)"):
                fn(_t(y), _t(y_len))
        assert model.to_counts() == counts                                       # the refused update counted nothing
        y[0, 2] = 5
        assert torch.equal(model.calculate_ce_loss(_t(y), _t(y_len)), want)


# ----------------------------------------------------------------------------- probabilities
@pytest.mark.parametrize("case,rows", [(NC.CASES[1], None), (NC.CASES[2], None), (NC.CASES[4], 8)], ids=["n3_v7", "n4_v30", "n3_v2350_8"])
def test_probabilities(dev, case, rows):
    N, V, B, L = case
    (ty, tl), (ey, el) = NC.case_data(case)
    ey, el = ey[:rows], el[:rows]
    model = _trained(case, dev)
    rest = NC.Model(N, V, NC.count_tables(ty, tl, N, V))
    for alpha in NC.ALPHAS:
        got_dev = model.calculate_probs(_t(ey), _t(el), alpha=alpha)
        assert torch.equal(got_dev, model.calculate_probs(_t(ey), _t(el), alpha=alpha))          # determinism
        got = got_dev.cpu().numpy()
        want = rest.probs(ey, el, alpha)
        assert got.shape == want.shape == (len(ey), L - 1, V) and got.dtype == np.float32
        d = NC.ulp_distance(got, want.astype(np.float32))
        inside = np.arange(1, L)[None, :] < el[:, None]
        print(f"[ngram probs {NC.case_name(case)} alpha {alpha}] bit-equal {float((d[inside] == 0).mean()):.4f}, worst {int(d.max())} ulp")
        assert d.max() <= 1 and np.all(got[~inside] == 0) and np.all(got[inside] > 0)
        loss = model.calculate_ce_loss(_t(ey), _t(el), alpha=alpha).cpu().numpy().astype(np.float64)
        at = np.take_along_axis(got.astype(np.float64), ey[:, 1:, None], axis=2)[..., 0]
        err = np.abs(-np.log(at[inside]) - loss[inside])
        assert np.all(err <= 2.0 ** -22 * np.maximum(1.0, loss[inside]))


# ----------------------------------------------------------------------------- processing
V_TOY, L_TOY = 7, 6


@pytest.fixture(scope="module")
def toy(dev):
    """Case (3, 7, 12, 6) as two data-module batches each, its n-gram model built by processing.build_ngram_model, the tag lists
    and the restatement."""
    from analysis_tools import processing as P
    case = NC.CASES[1]
    N, V, B, L = case
    (ty, tl), (ey, el) = NC.case_data(case)
    as_batches = lambda y, n: [(torch.zeros(b - a, 4), _t(y[a:b]), _t(n[a:b]), [["w"]] * (b - a)) for a, b in ((0, 5), (5, B))]   # noqa: E731
    model = P.build_ngram_model(N, V, as_batches(ty, tl), device=dev)
    tags = [["NN" if (b + i) % 3 else "VB" for i in range(int(n))] for b, n in enumerate(el)]
    tags[3] = tags[3][:-1] if len(tags[3]) > 1 else tags[3]                       # a tag list shorter than its utterance
    return P, model, as_batches(ey, el), tags, (ey, el), NC.Model(N, V, NC.count_tables(ty, tl, N, V))


def test_processing_run_model_and_losses(toy, dev):
    P, model, batches, _tags, (ey, el), rest = toy
    assert P.is_regressional(model) is True and model.to_counts() == NC.to_counts(rest.grams, V_TOY)
    want, _l64, _h = rest.ce_loss(ey, el, 0.1)
    _x, y, y_len, _raw = batches[0]
    outputs, loss = P.run_model(model, y, y_len)
    assert tuple(outputs.shape) == (5, L_TOY, 0) and tuple(loss.shape) == (5, L_TOY) and torch.all(loss[:, 0] == 0)
    _check_loss(loss[:, 1:], want[:5], el[:5], L_TOY, "run_model")
    outputs, loss, logits, attns, labels = P.run_model(model, y, y_len, return_all=True)
    assert attns is None and torch.equal(labels.cpu(), y[:, 1:]) and tuple(logits.shape) == (5, L_TOY - 1, V_TOY)
    assert torch.equal(logits, model.calculate_probs(y, y_len).log())
    o1, l1 = P.run_model(model, y[1], y_len[1], single_example=True)
    assert tuple(o1.shape) == (L_TOY, 0) and torch.equal(l1, loss[1])
    sums = P.get_model_losses_on_batches(model, batches)
    rows = torch.cat([P.run_model(model, b[1], b[2])[1] for b in batches]).sum(-1)
    assert torch.equal(sums, rows) and tuple(sums.shape) == (12,)
    per_example = list(P.run_model_on_data(model, batches))
    assert len(per_example) == 12 and torch.equal(per_example[6][5].cpu(), P.run_model(model, batches[1][1], batches[1][2])[1][1].cpu())


def test_processing_items(toy, dev):
    P, model, batches, tags, (ey, el), rest = toy
    items = P.get_model_items(model, batches, tags)
    want32, _l64, _h = rest.ce_loss(ey, el, 0.1)
    want = {}
    for b, t in enumerate(tags):
        for l, tag in enumerate(t):
            e = want.setdefault((int(ey[b, l]), tag), [0, 0.0])
            e[0] += 1
            e[1] += float(want32[b, l - 1]) if l else 0.0
    assert [tuple(k) for k in items.token_pos_items] == sorted(want) and items.all_token_items is None
    for key, value in items.token_pos_items.items():
        cnt, loss = want[tuple(key)]
        assert int(value.cnt) == cnt and value.vector.shape == (0,) and value.embedding is None
        # float64 sums of float32 terms that are each within 1 ulp (2^-23 relative) of the restatement's
        assert abs(float(value.loss) - loss) <= 2.0 ** -22 * max(loss, 1.0)
    assert all(v.vector.shape == (0,) and v.embedding is None for v in items.token_items.values())
    assert sum(int(v.cnt) for v in items.token_items.values()) == sum(len(t) for t in tags)
    assert [len(l) for l in items.losses] == el.tolist()
    assert all(np.array_equal(l[1:], model.calculate_ce_loss(_t(ey), _t(el)).cpu().numpy()[b, :len(l) - 1]) and l[0] == 0
               for b, l in enumerate(items.losses))


def test_processing_top_predictions_with_ties(toy, dev):
    P, model, batches, tags, (ey, el), rest = toy
    k = V_TOY                                                                     # the whole order: ids 0 and 1 are never seen and tie
    want = rest.probs(ey, el, 0.1)
    w32 = want.astype(np.float32)
    got = list(P.iter_top_predictions(model, batches, tags, top_k=k))
    assert [(u, l) for u, l, *_r in got] == [(u, l) for u, t in enumerate(tags) for l in range(len(t))]
    plain = P.get_model_top_predictions(model, batches, tags, top_k=k)
    assert len(plain) == len(got) and all(a[2] == b[0] for a, b in zip(got, plain))
    probs = P.get_model_probs(model, batches, tags)
    assert [p[0] for p in probs] == [g[2] for g in got]
    ties = 0
    for (u, l, key, label_prob, top_prob, top_idx), (_k, row) in zip(got, probs):
        assert key == P.Key(int(ey[u, l]), tags[u][l]) and row.shape == (V_TOY,)
        if l == 0:                                                                # predicts nothing: the top-k of a zero row
            assert label_prob == 0 and np.all(top_prob == 0) and top_idx.tolist() == list(range(k)) and np.all(row == 0)
            continue
        assert NC.ulp_distance(row, w32[u, l - 1]).max() <= 1
        order = np.lexsort((np.arange(V_TOY), -row.astype(np.float64)))[:k]       # (probability desc, index asc) of the device's row
        assert top_idx.tolist() == order.tolist() and np.array_equal(top_prob, row[order]) and label_prob == row[ey[u, l]]
        # and of the restatement's row, wherever one float32 step cannot change the order
        worder = np.lexsort((np.arange(V_TOY), -w32[u, l - 1].astype(np.float64)))
        ws = w32[u, l - 1][worder]
        if np.all((ws[:-1] == ws[1:]) | (NC.ulp_distance(ws[:-1], ws[1:]) > 2)):
            assert top_idx.tolist() == worder[:k].tolist()
        ties += int(np.any(top_prob[:-1] == top_prob[1:]))
    assert ties > 0                                                               # V = 7: equal back-off scores occur (input condition)


def test_word_statistics_main_with_ngram(tmp_path, dev):
    from analysis_tools import word_statistics as WS
    common = ["--random_init", "--dataset", "synthetic", "--split", "val", "--batch_size", "8", "--top_k", "3"]
    WS.main(WS.parser().parse_args(common + ["--out", str(tmp_path / "a")]))
    WS.main(WS.parser().parse_args(common + ["--out", str(tmp_path / "b"), "--ngram", "3", "--ngram_alpha", "0.2"]))
    old = ("token_items.csv", "token_vectors.npy", "losses.npy", "top_predictions.csv")
    new = ("ngram_token_items.csv", "ngram_losses.npy", "ngram_top_predictions.csv")
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(old)
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(old + new)
    for name in old:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    with open(tmp_path / "b" / "ngram_token_items.csv") as f:
        rows = list(csv.reader(f))
    with open(tmp_path / "b" / "token_items.csv") as f:
        lm_rows = list(csv.reader(f))
    assert rows[0] == lm_rows[0] and [r[:3] for r in rows] == [r[:3] for r in lm_rows]          # the same words, tags and counts
    losses, lm_losses = np.load(tmp_path / "b" / "ngram_losses.npy"), np.load(tmp_path / "b" / "losses.npy")
    assert losses.shape == lm_losses.shape and np.all(losses[:, 0] == 0) and np.all(losses[:, 1:] > 0)
    with open(tmp_path / "b" / "ngram_top_predictions.csv") as f:
        pred = list(csv.reader(f))
    with open(tmp_path / "b" / "top_predictions.csv") as f:
        lm_pred = list(csv.reader(f))
    assert pred[0] == lm_pred[0] and [p[:4] for p in pred] == [p[:4] for p in lm_pred]
    assert all(float(p[6]) >= float(p[8]) >= float(p[10]) for p in pred[1:])
