"""CPU: tests/golden/word_statistics.npz against a float64 restatement of the reference's arithmetic from the formula-filled
weights (5e-6 relative, the bound oracle/gen_golden.py holds restatements to), the arrangement of the fixture's data, and the
validity of the top-k inputs of test_word_statistics_gpu.py for exact selection."""
import numpy as np
import pytest
import torch

import word_statistics_common as WC

TOL = 5e-6
TOPK_CASES = [(77, 50, 5), (77, 50, 1), (33, 2350, 16), (5, 64, 16)]


@pytest.fixture(scope="module")
def fx():
    return WC.fixture()


def test_data_arrangement(fx):
    z, batches, pos_tags = fx
    assert [tuple(b[1].shape) for b in batches] == [(7, 9), (5, 6)] and len(pos_tags) == 12
    lens = torch.cat([b[2] for b in batches]).tolist()
    assert min(lens) == 2 and max(lens) == 9 and set(t for tags in pos_tags for t in tags) == {".", "NN", "VB", "DT"}
    assert [len(t) for t in pos_tags] == [n - 2 if i == 3 else n for i, n in enumerate(lens)]     # one tag list is short
    keys, cnt, _loss, _vec = WC.stored_items(z, "plain", "token_pos_items")
    table = dict(zip(keys, cnt.tolist()))
    assert table[(30, "NN")] == table[(30, "VB")] == 1 and sum(c for (tok, _t), c in table.items() if tok == 40) == 1
    words, _c, _l, _v = WC.stored_items(z, "plain", "token_items")
    assert (30, "VB") in words and (30, "NN") not in words                        # the tie goes to the larger tag
    assert keys == sorted(keys) and words == sorted(words) and table[(2, ".")] == 12 and table[(3, ".")] == 11


@pytest.mark.parametrize("name", ["plain", "captioning"])
def test_restatement_reproduces_the_reference(fx, name):
    z, batches, pos_tags = fx
    losses, token_pos, probs = WC.restate(WC.toy_weights(name == "captioning"), batches, pos_tags, name == "captioning")
    assert WC.err(z[f"{name}.losses"], losses) < TOL
    for table, mine in (("token_pos_items", token_pos), ("token_items", WC.merge_by_word(token_pos))):
        keys, cnt, loss, vec = WC.stored_items(z, name, table)
        assert keys == sorted(mine)
        assert cnt.tolist() == [mine[k][0] for k in keys]
        assert WC.err(loss, torch.stack([mine[k][1] for k in keys])) < TOL
        assert WC.err(vec, torch.stack([mine[k][2] for k in keys])) < TOL
    assert list(zip(z[f"{name}.probs.token_id"].tolist(), z[f"{name}.probs.pos"].tolist())) == [k for k, _p in probs]
    assert WC.err(z[f"{name}.probs"], torch.stack([p for _k, p in probs])) < TOL
    p64 = torch.stack([p for _k, p in probs]).sort(1, descending=True).values[:, :int(z["exact_k"]) + 1]
    live = p64[:, 0] > 0                                                          # (the leading zero rows predict nothing)
    assert int((~live).sum()) == 12 and float((p64[live, :-1] - p64[live, 1:]).min()) > 1e-4


@pytest.mark.parametrize("R,V,k", TOPK_CASES)
def test_topk_inputs_are_valid_for_exact_selection(R, V, k):
    logits, labels = WC.topk_logits(R, V, k, seed=R + V + k)
    _tp, idx, p, gap = WC.topk_reference(logits, k)
    assert gap > 1e-4, gap
    assert idx.shape == (R, k) and all(len(set(r)) == k for r in idx.tolist())
    assert int((labels == 0).sum()) >= 1 and int((labels != 0).sum()) >= 1
    bound, measured = WC.softmax_bound(logits)
    print(f"torch fp32 softmax vs float64 at ({R}, {V}): {measured:.2e} -> bound {bound:.2e}")
    assert 0 < measured < 1e-5
