"""CPU: vit_discard_common.discard_ref, the yardstick of tests/test_vit_discard_gpu.py, against a brute-force loop that follows the
definition word by word, on hand-made matrices: a tie group that straddles the threshold (the lowest indices go), element 0 as the
smallest value (kept, and only k - 1 others zeroed), k = 0 and k = M - 1."""
import pytest
import torch

from vit_discard_common import discard_ref


def _brute(F, k):
    """One matrix: pick the smallest remaining value k times, the lowest index among equals; zero the picks other than index 0."""
    vals = F.reshape(-1).tolist()
    left = list(range(len(vals)))
    out = list(vals)
    for _ in range(k):
        best = left[0]
        for i in left[1:]:
            if vals[i] < vals[best]:                        # strict: an equal value at a higher index does not replace it
                best = i
        left.remove(best)
        if best != 0:
            out[best] = 0.0
    return torch.tensor(out, dtype=F.dtype).reshape(F.shape)


TIES = torch.tensor([[0.50, 0.20, 0.30],
                     [0.20, 0.10, 0.20],
                     [0.40, 0.20, 0.60]])                   # four 0.20 at flat 1, 3, 5, 7
ZERO_MIN = torch.tensor([[0.01, 0.30, 0.20, 0.25],
                         [0.05, 0.40, 0.02, 0.35],
                         [0.50, 0.03, 0.45, 0.60],
                         [0.70, 0.80, 0.04, 0.90]])         # element 0 is the minimum


def test_tie_group_straddling_the_threshold():
    got = discard_ref(TIES, 3)                              # 0.10, then the 0.20 at flat 1 and 3; those at 5 and 7 stay
    want = torch.tensor([[0.50, 0.0, 0.30], [0.0, 0.0, 0.20], [0.40, 0.20, 0.60]])
    assert torch.equal(got, want) and torch.equal(got, _brute(TIES, 3))
    assert torch.equal(discard_ref(TIES, 4), torch.tensor([[0.50, 0.0, 0.30], [0.0, 0.0, 0.0], [0.40, 0.20, 0.60]]))


def test_element_zero_is_kept_but_counted():
    got = discard_ref(ZERO_MIN, 3)                          # picks 0.01 (kept), 0.02, 0.03: two zeros, not three
    assert got[0, 0] == ZERO_MIN[0, 0] and int((got == 0).sum()) == 2
    assert got[1, 2] == 0 and got[2, 1] == 0 and got[3, 2] == ZERO_MIN[3, 2]
    assert torch.equal(got, _brute(ZERO_MIN, 3))
    assert torch.equal(discard_ref(ZERO_MIN, 1), ZERO_MIN)


@pytest.mark.parametrize("F", [TIES, ZERO_MIN], ids=["3x3", "4x4"])
def test_every_k_against_the_brute_force_loop(F):
    M = F.numel()
    assert torch.equal(discard_ref(F, 0), F)                # k = 0: nothing
    last = discard_ref(F, M - 1)                            # k = M - 1: the maximum and element 0 are all that is left
    keep = {0, int(F.reshape(-1).argmax())}
    assert {i for i in range(M) if last.reshape(-1)[i] != 0} == keep
    for k in range(M):
        assert torch.equal(discard_ref(F, k), _brute(F, k)), k


def test_matrices_of_a_batch_are_selected_one_by_one_and_the_input_is_left_alone():
    both = torch.stack([TIES, TIES.flip(0).contiguous()])[None]            # [1, 2, 3, 3]
    before = both.clone()
    got = discard_ref(both, 5)
    assert torch.equal(both, before)
    for b in range(2):
        assert torch.equal(got[0, b], _brute(both[0, b], 5))
    got64 = discard_ref(both.double(), 5)
    assert got64.dtype == torch.float64 and torch.equal(got64.float(), got)
