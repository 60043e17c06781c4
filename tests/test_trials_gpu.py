"""GPU: cvcl_trial_scores (csrc/trials.hip) against float64 on seeded inputs.

Inputs.  Per D one query table [NQ = 5, D] and one candidate table [NC = 19, D] of fp32 normal deviates scaled by D^(-1/4) (a dot
product is then of order 1), and per (T, n) an index table whose rows repeat all over (T up to 1000 trials draw from 5 and 19 rows)
but, in the main table, never inside a trial.  A trial's float64 logits are entries of ONE 5 x 19 matrix per (D, scale), computed
once per module and never changed.

Logit bound (derived, not tuned).  The kernel's logit is fl(scale32 * fl(sum of D fp32 products, by fma, in some order)).  Any
order of an fp32 sum of D products is within (D - 1 + 1) u sum_i |q_i k_i| of the exact sum to first order (u = 2^-24; one rounding
per addition, one per product -- none with fma); the multiplication by the scale adds u, and scale32 = expf(log_scale) is within
1 ulp <= 2 u of exp(log_scale) (HIP math accuracy table: expf 1 ulp).  Together at most (D + 3) u, stated with one to spare:
    |logit - logit64| <= (D + 4) 2^-24 scale sum_i |q_i k_i|          evaluated per entry in float64.

Probability bound.  With every logit of a trial within B (the trial's largest logit bound) of its float64 value, each soft-max
ratio p'_j / p_j and (1 - p'_j) / (1 - p_j) lies in [e^(-2B), e^(2B)], so |p'_j - p_j| <= min(p_j, 1 - p_j) (e^(2B) - 1) <= 2 B as long
as B < 0.5 (asserted).  On top of that the kernel's own fp32 evaluation of softmax(logits32), p_j = fl(e_j / s) with
e_j = expf(fl(l_j - m)) and s = the e_k added in order, s >= 1 because the maximum's term is exactly 1:
    the subtraction rounds by <= u |x_j| (x_j = l_j - m <= 0), which moves e_j by <= u |x_j| e^(x_j) <= u / e absolutely,
    expf is within 1 ulp (HIP math accuracy table), a relative 2 u on e_j and on every term of s,
    the n - 1 additions of positive terms add a relative (n - 1) u to s, the terms' own shifts at most n u / e in all,
    the division is correctly rounded (IEEE division is the default of hipcc without -ffast-math): a relative u,
so |p_j - softmax(logits32)_j| <= p_j (2 + 2 + (n - 1) + 1) u + (1 + n) u / e <= (2 n + 8) u.  The asserted bound is
    |prob - prob64| <= 2 B + (2 n + 8) 2^-24.

pred must be the float64 arg-max wherever the float64 top-two gap exceeds 2 B.  SEEDS holds, per D, a seed (found on the CPU when
this file was written, by trying 0, 1, 2, ...) for which ALL 19 logits of every query row are more than twice the row's largest
bound apart; the ratio does not depend on the scale.  So no trial of any table is left out, and the test asserts that.

Ties: a trial whose c_idx repeats a row has bitwise-equal logits there, and pred is the lowest position of the maximum.  Invalid
indices (-1, NQ, NC -- never dereferenced by the kernel, that is what is tested; no index is passed that the kernel would read out of
bounds) give NaN / -1 for that trial alone; the outputs sit inside larger sentinel-filled allocations whose other words must keep
the sentinel.  A trial's bits do not depend on T."""
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

NQ, NC = 5, 19
DS = (1, 3, 37, 64, 255, 257, 512, 768)
NS = (1, 2, 4, 5, 16)
TS = (1, 63, 64, 65, 1000)
LOG_SCALE = -math.log(0.07)
SEEDS = {1: 0, 3: 0, 37: 0, 64: 0, 255: 0, 257: 1, 512: 0, 768: 2}
U = 2.0 ** -24
PAD = 5


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    _hip.load()
    return _hip


def features(D):
    g = torch.Generator().manual_seed(1000 * D + SEEDS[D])
    return torch.randn(NQ, D, generator=g) * D ** -0.25, torch.randn(NC, D, generator=g) * D ** -0.25


def reference(D, log_scale):
    """-> (logit64 [NQ, NC], bound [NQ, NC]) in float64 from the fp32 inputs"""
    q, c = (t.double() for t in features(D))
    scale = math.exp(float(np.float32(log_scale))) if log_scale is not None else 1.0
    return scale * q @ c.t(), (D + 4) * U * scale * q.abs() @ c.abs().t()


_REF = {}


def ref(D, log_scale):
    if (D, log_scale) not in _REF:
        _REF[D, log_scale] = reference(D, log_scale)
    return _REF[D, log_scale]


def index_table(T, n, seed):
    """q_idx [T] into the 5-row table, c_idx [T, n] into the 19-row table, int32, no row twice inside a trial"""
    g = torch.Generator().manual_seed(seed)
    q_idx = torch.randint(0, NQ, (T,), generator=g, dtype=torch.int32)
    c_idx = torch.stack([torch.randperm(NC, generator=g)[:n] for _ in range(T)]).to(torch.int32)
    return q_idx, c_idx


def run(H, dev, q, c, q_idx, c_idx, log_scale, ld_pad=0, want_logits=True, out=None):
    """the C entry on device copies; rows of width D inside allocations of width D + ld_pad -> (logits, probs, pred) on the host"""
    D = q.shape[1]
    qd = torch.full((q.shape[0], D + ld_pad), 7.0, device=dev)
    cd = torch.full((c.shape[0], D + ld_pad), -7.0, device=dev)
    qd[:, :D], cd[:, :D] = q.to(dev), c.to(dev)
    qi, ci = q_idx.to(dev).contiguous(), c_idx.to(dev).contiguous()
    T, n = c_idx.shape
    ls = torch.tensor(log_scale, dtype=torch.float32, device=dev) if log_scale is not None else None
    if out is None:
        out = (torch.zeros(T, n, device=dev), torch.zeros(T, n, device=dev), torch.zeros(T, dtype=torch.int32, device=dev))
    logits, probs, pred = out
    rc = H.lib().cvcl_trial_scores(qd.data_ptr(), D + ld_pad, q.shape[0], cd.data_ptr(), D + ld_pad, c.shape[0], D, qi.data_ptr(),
                                   ci.data_ptr(), T, n, None if ls is None else ls.data_ptr(),
                                   logits.data_ptr() if want_logits else None, probs.data_ptr(), pred.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    H.check(rc, "cvcl_trial_scores")
    torch.cuda.synchronize()
    return logits.cpu(), probs.cpu(), pred.cpu()


def check_against_float64(D, log_scale, q_idx, c_idx, logits, probs, pred):
    l64, b64 = ref(D, log_scale)
    qi, ci = q_idx.long(), c_idx.long()
    want, bound = l64[qi[:, None], ci], b64[qi[:, None], ci]
    err = (logits.double() - want).abs()
    assert bool((err <= bound).all()), (D, float((err / bound).max()))
    B = bound.max(dim=1).values
    assert float(B.max()) < 0.5
    n = ci.shape[1]
    p64 = torch.softmax(want, dim=1)
    perr = (probs.double() - p64).abs()
    assert bool((perr <= (2 * B + (2 * n + 8) * U)[:, None]).all()), (D, n, float(perr.max()))
    assert bool(((probs.sum(1) - 1).abs() <= (n + 2) * 2 * U).all())
    if n > 1:
        top = want.topk(2, dim=1).values
        decided = (top[:, 0] - top[:, 1]) > 2 * B
    else:
        decided = torch.ones(len(qi), dtype=torch.bool)
    assert bool(decided.all()), (D, n, int((~decided).sum()))              # the seeds leave no trial out
    assert torch.equal(pred.long(), want.argmax(dim=1))


def test_seeds_separate_every_pair():
    """CPU arithmetic only (it sits here because it is about this file's tables): what the docstring says of SEEDS"""
    for D in DS:
        l64, b64 = ref(D, LOG_SCALE)
        for lt, bt in ((l64, b64), (l64.t(), b64.t())):      # (and with the roles swapped: every column's 5 logits)
            for r in range(lt.shape[0]):
                v = lt[r].sort().values
                assert float((v[1:] - v[:-1]).min()) > 2 * float(bt[r].max()), (D, r)


@gpu
@pytest.mark.parametrize("log_scale", [None, LOG_SCALE], ids=["noscale", "scale"])
@pytest.mark.parametrize("ld_pad", [0, PAD])
@pytest.mark.parametrize("D", DS)
def test_values_against_float64(H, dev, D, ld_pad, log_scale):
    q, c = features(D)
    for n in NS:
        for T in TS:
            q_idx, c_idx = index_table(T, n, 17 * T + n)
            check_against_float64(D, log_scale, q_idx, c_idx, *run(H, dev, q, c, q_idx, c_idx, log_scale, ld_pad))


@gpu
def test_roles_swapped_and_logits_optional(H, dev):
    """the 19-row table as the query (text trials: a frame against words), and logits = NULL writes the same probs and pred"""
    D, T, n = 257, 65, 4
    small, large = features(D)
    g = torch.Generator().manual_seed(5)
    q_idx = torch.randint(0, NC, (T,), generator=g, dtype=torch.int32)
    c_idx = torch.stack([torch.randperm(NQ, generator=g)[:n] for _ in range(T)]).to(torch.int32)
    logits, probs, pred = run(H, dev, large, small, q_idx, c_idx, LOG_SCALE, PAD)
    l64, b64 = (t.t() for t in ref(D, LOG_SCALE))
    want, bound = l64[q_idx.long()[:, None], c_idx.long()], b64[q_idx.long()[:, None], c_idx.long()]
    assert bool(((logits.double() - want).abs() <= bound).all())
    assert torch.equal(pred.long(), want.argmax(dim=1))
    _, probs2, pred2 = run(H, dev, large, small, q_idx, c_idx, LOG_SCALE, PAD, want_logits=False)
    assert torch.equal(probs.view(torch.int32), probs2.view(torch.int32)) and torch.equal(pred, pred2)


@gpu
@pytest.mark.parametrize("D", [37, 768])
def test_ties_go_to_the_lowest_position(H, dev, D):
    q, c = features(D)
    l64, _ = ref(D, LOG_SCALE)
    T = NQ * 4
    q_idx = torch.arange(T, dtype=torch.int32) % NQ
    best = l64.argmax(dim=1)[q_idx.long()].to(torch.int32)                 # the row that wins against every other, per query
    other = (best + 1 + torch.arange(T, dtype=torch.int32) % (NC - 1)) % NC
    c_idx = torch.stack([other, best, best, other, best], dim=1).contiguous()
    logits, probs, pred = run(H, dev, q, c, q_idx, c_idx, LOG_SCALE)
    bits = logits.view(torch.int32)
    assert torch.equal(bits[:, 1], bits[:, 2]) and torch.equal(bits[:, 1], bits[:, 4]) and torch.equal(bits[:, 0], bits[:, 3])
    assert torch.equal(probs.view(torch.int32)[:, 1], probs.view(torch.int32)[:, 2])
    assert bool((pred == 1).all())
    c_idx = torch.stack([best, best, other], dim=1).contiguous()           # and at position 0
    assert bool((run(H, dev, q, c, q_idx, c_idx, None)[2] == 0).all())
    c_idx = best[:, None].repeat(1, 16).contiguous()                       # all 16 alike: uniform, position 0
    logits, probs, pred = run(H, dev, q, c, q_idx, c_idx, LOG_SCALE)
    assert bool((pred == 0).all()) and bool((probs == 1.0 / 16).all())


@gpu
def test_invalid_indices_are_never_dereferenced(H, dev):
    D, T, n, guard = 255, 9, 4, 64
    q, c = features(D)
    q_idx, c_idx = index_table(T, n, 3)
    good = run(H, dev, q, c, q_idx, c_idx, LOG_SCALE, PAD)
    bad_q, bad_c = q_idx.clone(), c_idx.clone()
    bad_q[2], bad_q[4] = -1, NQ
    bad_c[6, 2], bad_c[7, 0], bad_c[4, 3] = NC, -1, NC
    bad = [2, 4, 6, 7]
    SENT_F, SENT_I = 12345.0, 0x5A5A5A5A
    big = [torch.full((guard + T * n + guard,), SENT_F, device=dev), torch.full((guard + T * n + guard,), SENT_F, device=dev),
           torch.full((guard + T + guard,), SENT_I, dtype=torch.int32, device=dev)]
    out = (big[0][guard:guard + T * n].view(T, n), big[1][guard:guard + T * n].view(T, n), big[2][guard:guard + T])
    logits, probs, pred = run(H, dev, q, c, bad_q, bad_c, LOG_SCALE, PAD, out=out)
    for t in range(T):
        if t in bad:
            assert bool(torch.isnan(logits[t]).all()) and bool(torch.isnan(probs[t]).all()) and int(pred[t]) == -1, t
        else:                                              # the neighbours are exact
            assert torch.equal(logits[t].view(torch.int32), good[0][t].view(torch.int32)), t
            assert torch.equal(probs[t].view(torch.int32), good[1][t].view(torch.int32)) and pred[t] == good[2][t], t
    for b, sent in zip(big, (SENT_F, SENT_F, SENT_I)):     # nothing beside the outputs was touched
        b = b.cpu()
        assert bool((b[:guard] == sent).all()) and bool((b[-guard:] == sent).all())
    # without a logits buffer the guard is the same
    big[1].fill_(SENT_F)
    _, probs2, pred2 = run(H, dev, q, c, bad_q, bad_c, LOG_SCALE, PAD, want_logits=False, out=out)
    assert torch.equal(torch.isnan(probs2), torch.isnan(probs)) and torch.equal(pred2, pred)


@gpu
def test_a_trial_does_not_depend_on_T(H, dev):
    from multimodal import trials
    for D, n in ((768, 4), (37, 16)):
        q, c = features(D)
        q_idx, c_idx = index_table(1000, n, 11)
        logits, probs, pred = run(H, dev, q, c, q_idx, c_idx, LOG_SCALE, PAD)
        for t in (0, 1, 2, 3, 501, 998, 999):
            l1, p1, d1 = run(H, dev, q, c, q_idx[t:t + 1], c_idx[t:t + 1], LOG_SCALE, PAD)
            assert torch.equal(l1.view(torch.int32)[0], logits.view(torch.int32)[t]), (D, t)
            assert torch.equal(p1.view(torch.int32)[0], probs.view(torch.int32)[t]) and int(d1[0]) == int(pred[t]), (D, t)
        # the host wrapper: the same bits, fetched in one copy; strided views are read in place
        wide = torch.zeros(NC, D + PAD, device=dev)
        wide[:, :D] = c.to(dev)
        p, d, l = trials.score_trials(q.to(dev), wide[:, :D], q_idx, c_idx, torch.tensor(LOG_SCALE, dtype=torch.float32, device=dev),
                                      return_logits=True)
        assert not p.is_cuda and p.dtype == torch.float32 and d.dtype == torch.int32
        assert torch.equal(p.view(torch.int32), probs.view(torch.int32)) and torch.equal(d, pred)
        assert torch.equal(l.cpu().view(torch.int32), logits.view(torch.int32))
    p, d = trials.score_trials(q.to(dev), c.to(dev), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32))
    assert p.shape == (0, 4) and d.shape == (0,)
