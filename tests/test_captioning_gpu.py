"""GPU: beam-search decoding of the LSTM language model (csrc/textgen.hip, csrc/lstm.hip, ops.beam_search_lstm, LanguageModel.beam_search_decode).

- cvcl_beam_step alone at B = 256, V = 2350 against a float64 restatement of one step of the reference algorithm written here;
- the whole decode against the reference's own beam_search_decode (tests/golden/captioning_beam.npz, tools/gen_golden_captioning.py);
- the image-initialised LSTM (captioning) against a float64 nn.LSTM; determinism."""
import argparse
import contextlib
import io
import math
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

V_SAYCAM = 2350
EOS = 3


# ---------------------------------------------------------------------------------------------------------------- step restatement
def _f32(x):
    return float(np.float32(x))


def _penal(score):
    return float(np.float32(np.float32(score) + np.float32(-1e7)))


def restate_step(logits, alive_lp, fin_scores, fin_flags, alive_seq, fin_seq, h, c, step, alpha, T):
    """One decode step in float64 from the algorithm: candidates = (log_softmax + alive log-prob) / lp, top 2K by (score desc,
    flat index asc); alive = top K of score - 1e7 [finished]; finished = top K of [finished ; score - 1e7 [not finished]];
    sequences and states gathered by parent.  Returns None when the stop test holds."""
    B, K, V = logits.shape
    lp = _f32(((5.0 + step + 1) / 6.0) ** alpha)
    max_lp = _f32(((5.0 + T) / 6.0) ** alpha)
    met = (fin_scores.max(1).values > alive_lp[:, 0] / max_lp).all()
    if bool(met):
        return None
    lg = logits.double()
    logp = lg - torch.logsumexp(lg, -1, keepdim=True)
    scores = ((logp + alive_lp.double()[:, :, None]) / lp).reshape(B, K * V)
    out = dict(alive_lp=torch.empty(B, K, dtype=torch.float64), fin=torch.empty(B, K, dtype=torch.float64),
               flags=torch.empty(B, K, dtype=torch.int32), alive_seq=alive_seq.clone(), fin_seq=fin_seq.clone(),
               h=torch.empty_like(h), c=torch.empty_like(c), tok=torch.empty(B * K, dtype=torch.int64), cand=[])
    for b in range(B):
        s = scores[b]
        order = torch.argsort(-s, stable=True)[:2 * K].tolist()                 # (score desc, index asc)
        cs = [float(s[f]) for f in order]
        beam = [f // V for f in order]
        tok = [f % V for f in order]
        fin_c = [t == EOS for t in tok]
        out["cand"].append(order)
        # the -1e7 penalty is added to fp32 scores: at that magnitude the fp32 sum decides the order of penalised slots
        a_key = [(-(_penal(cs[r]) if fin_c[r] else cs[r]), r) for r in range(2 * K)]
        a_sel = [r for _, r in sorted(a_key)[:K]]
        f_all = [float(fin_scores[b, j]) for j in range(K)] + [cs[r] if fin_c[r] else _penal(cs[r]) for r in range(2 * K)]
        f_sel = [j for _, j in sorted((-v, j) for j, v in enumerate(f_all))[:K]]
        for k, r in enumerate(a_sel):
            p = beam[r]
            out["alive_lp"][b, k] = cs[r] * lp
            out["alive_seq"][b, k, :step + 1] = alive_seq[b, p, :step + 1]
            out["alive_seq"][b, k, step + 1] = tok[r]
            out["h"][b * K + k] = h[b * K + p]
            out["c"][b * K + k] = c[b * K + p]
            out["tok"][b * K + k] = tok[r]
        for k, j in enumerate(f_sel):
            out["fin"][b, k] = f_all[j]
            if j < K:
                out["flags"][b, k] = fin_flags[b, j]
                out["fin_seq"][b, k, :step + 1] = fin_seq[b, j, :step + 1]
                out["fin_seq"][b, k, step + 1] = 0
            else:
                r = j - K
                out["flags"][b, k] = int(fin_c[r])
                out["fin_seq"][b, k, :step + 1] = alive_seq[b, beam[r], :step + 1]
                out["fin_seq"][b, k, step + 1] = tok[r]
    return out


def _step_inputs(B, K, V, step, seed, T=25, Hd=64):
    """Logits whose candidates are well separated: every beam holds a permutation of the same values -0.01 j (so the beams share
    their log-sum-exp) and the alive log-probs differ by fractions of 0.01 / (K + 1), so any two scores are >= 0.01 / (K + 1) / lp
    apart.  Odd items carry <eos> among the strongest tokens of every beam, so candidates finish; at step 0 every beam but the first
    is -inf, as a decode starts."""
    g = torch.Generator().manual_seed(seed)
    vals = -0.01 * torch.arange(V, dtype=torch.float64)
    logits = torch.empty(B, K, V)
    for b in range(B):
        for k in range(K):
            perm = torch.randperm(V, generator=g)
            if b % 2:
                v = int((perm == k % 3).nonzero()[0, 0])
                perm[v], perm[EOS] = perm[EOS].clone(), perm[v].clone()
            logits[b, k] = vals[perm].float()
    if step == 0:
        alive_lp = torch.full((B, K), -math.inf)
        alive_lp[:, 0] = 0.
        fin = torch.full((B, K), -1e7)
        flags = torch.zeros(B, K, dtype=torch.int32)
    else:
        frac = torch.stack([torch.randperm(K, generator=g) for _ in range(B)]).float() * (0.01 / (K + 1))
        alive_lp = -2.0 - frac - 0.01 * torch.randint(0, 4, (B, K), generator=g).float()
        alive_lp = alive_lp.sort(1, descending=True).values
        fin = torch.full((B, K), -1e7)
        flags = torch.zeros(B, K, dtype=torch.int32)
        some = torch.arange(B) % 3 == 0                                           # a third of the items already hold finished beams
        fin[some, 0] = -6.0 - torch.rand(int(some.sum()), generator=g)
        flags[some, 0] = 1
    alive_seq = torch.randint(4, V, (B, K, T + 1), generator=g)
    alive_seq[:, :, step + 1:] = 0
    fin_seq = torch.randint(4, V, (B, K, T + 1), generator=g) * flags[:, :, None].long()
    fin_seq[:, :, step + 1:] = 0
    h = torch.randn(B * K, Hd, generator=g)
    c = torch.randn(B * K, Hd, generator=g)
    return logits, alive_lp, fin, flags, alive_seq, fin_seq, h, c


def _run_step(dev, logits, alive_lp, fin, flags, alive_seq, fin_seq, h, c, step, alpha, T, steps0=None):
    from multimodal import _hip as H
    B, K, V = logits.shape
    Hd = h.shape[1]
    d = lambda t: t.to(dev).contiguous()
    t = dict(logits=d(logits), a_in=d(alive_lp), a_out=torch.full((B, K), 7.0, device=dev), f_in=d(fin),
             f_out=torch.full((B, K), 7.0, device=dev), aseq=d(alive_seq), fseq=d(fin_seq), flags=d(flags), h=d(h), c=d(c),
             h_out=torch.zeros_like(d(h)), c_out=torch.zeros_like(d(c)), tok=torch.full((B * K,), -5, dtype=torch.int64, device=dev),
             steps=torch.full((1,), T if steps0 is None else steps0, dtype=torch.int32, device=dev))
    lib = H.lib()
    H.check(lib.cvcl_beam_step(H.ptr(t["logits"]), B, K, V, T, step, float(alpha), EOS, H.ptr(t["a_in"]), H.ptr(t["a_out"]),
                               H.ptr(t["f_in"]), H.ptr(t["f_out"]), H.ptr(t["aseq"]), H.ptr(t["fseq"]), H.ptr(t["flags"]),
                               H.ptr(t["h"]), H.ptr(t["c"]), H.ptr(t["h_out"]), H.ptr(t["c_out"]), Hd, H.ptr(t["tok"]),
                               H.ptr(t["steps"]), H.stream_ptr()), "cvcl_beam_step")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in t.items()}


def _check_separation(logits, alive_lp, step, alpha, K):
    """The inputs are a valid exact-selection test: in float64 the 2K + 1 best scores of every item are >= 1e-4 apart."""
    lp = _f32(((5.0 + step + 1) / 6.0) ** alpha)
    lg = logits.double()
    s = ((lg - torch.logsumexp(lg, -1, keepdim=True) + alive_lp.double()[:, :, None]) / lp).reshape(logits.shape[0], -1)
    top = s.topk(2 * K + 1, dim=1).values
    fin = top[:, :2 * K + 1]
    gaps = (fin[:, :-1] - fin[:, 1:])
    assert float(gaps[torch.isfinite(gaps)].min()) > 1e-4


@pytest.mark.parametrize("K", [3, 5, 16])
@pytest.mark.parametrize("step,alpha", [(0, 0.6), (7, 0.6), (12, 0.0)])
def test_beam_step_matches_float64_restatement(dev, K, step, alpha):
    B, V, T = 256, V_SAYCAM, 25
    inp = _step_inputs(B, K, V, step, seed=100 * K + step)
    _check_separation(inp[0], inp[1], step, alpha, K)
    got = _run_step(dev, *inp, step, alpha, T)
    ref = restate_step(*inp, step, alpha, T)
    assert ref is not None
    assert int(got["steps"][0]) == T                                   # not stopped
    assert torch.equal(got["aseq"], ref["alive_seq"])
    assert torch.equal(got["fseq"], ref["fin_seq"])
    assert torch.equal(got["flags"], ref["flags"])
    assert torch.equal(got["tok"], ref["tok"])
    assert torch.equal(got["h_out"], ref["h"]) and torch.equal(got["c_out"], ref["c"])
    assert bool(ref["flags"].any()) and bool((ref["flags"] == 0).any())   # finished candidates were in play
    for k_got, k_ref in (("a_out", "alive_lp"), ("f_out", "fin")):
        r = ref[k_ref]
        assert float(((got[k_got].double() - r).abs() / r.abs().clamp_min(1.0)).max()) < 1e-6, k_got
    assert torch.equal(got["a_in"], inp[1]) and torch.equal(got["f_in"], inp[2])   # the *_in halves are read only


def test_beam_step_stop_test(dev):
    """Every item's best finished score above its alive bound: the step is a no-op that carries the state over and records the
    step; with one item below the bound the step runs."""
    B, K, V, T, step, alpha = 256, 3, V_SAYCAM, 25, 9, 0.6
    inp = list(_step_inputs(B, K, V, step, seed=7))
    inp[2][:, 0] = -0.1                                                 # finished scores above every alive bound
    inp[3][:, 0] = 1
    assert restate_step(*inp, step, alpha, T) is None
    got = _run_step(dev, *inp, step, alpha, T)
    assert int(got["steps"][0]) == step
    assert torch.equal(got["a_out"], inp[1]) and torch.equal(got["f_out"], inp[2])
    assert torch.equal(got["aseq"], inp[4]) and torch.equal(got["fseq"], inp[5]) and torch.equal(got["flags"], inp[3])
    assert bool((got["tok"] == -5).all()) and float(got["h_out"].abs().sum()) == 0.0
    # an earlier recorded stop is kept (atomic minimum)
    assert int(_run_step(dev, *inp, step, alpha, T, steps0=4)["steps"][0]) == 4
    inp[2][B - 1, 0] = -1e7                                             # one item below its bound: the batch goes on
    inp[3][B - 1, 0] = 0
    ref = restate_step(*inp, step, alpha, T)
    got = _run_step(dev, *inp, step, alpha, T)
    assert int(got["steps"][0]) == T
    assert torch.equal(got["aseq"], ref["alive_seq"]) and torch.equal(got["fseq"], ref["fin_seq"])


# ---------------------------------------------------------------------------------------------------------------- whole decode
def _lm(dev, captioning, eos_bias=None, V=50, E=32):
    from multimodal.multimodal import LanguageModel, TextEncoder
    vocab = {"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, **{f"w{i}": i for i in range(4, V)}}
    args = argparse.Namespace(text_encoder="lstm", embedding_type="flat", embedding_dim=E, crange=1, dropout_i=0.0, dropout_o=0.0,
                              pos_embed_type="no_pos_embed", captioning=captioning, attention=False, attention_gate=False,
                              tie=True, bias=True)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(vocab, 2048, args)
        lm = LanguageModel(te, args)
    if eos_bias is not None:
        sys.path.insert(0, ROOT + "/tools")
        import gen_golden_captioning as G
        G.fill_text_encoder(te)
        with torch.no_grad():
            lm.output_layer.bias.copy_(G.output_bias(eos_bias))
    return te.to(dev).eval(), lm.to(dev).eval()


def test_decode_matches_reference_fixtures(dev):
    sys.path.insert(0, ROOT + "/tools")
    import gen_golden_captioning as G
    g = load_golden("captioning_beam")
    feats = g["image_features"].to(dev)
    cases = [str(c) for c in g["cases"]]
    assert len(cases) >= 24 and any(g[c + ".seq"].shape[2] < int(c.split("_t")[1]) + 1 for c in cases)
    models = {}
    for name in cases:
        kind, bias_name, k, a, t = name.split("_")
        K, alpha, T = int(k[1:]), float(a[1:]), int(t[1:])
        key = (kind, bias_name)
        if key not in models:
            models[key] = _lm(dev, kind == "cap", G.EOS_BIAS[bias_name])
        te, lm = models[key]
        with torch.no_grad():
            seq, score = lm.beam_search_decode(G.B, K, T, alpha, image_features=feats if kind == "cap" else None)
        ref_seq, ref_score = g[name + ".seq"], g[name + ".score"]
        assert tuple(seq.shape) == tuple(ref_seq.shape), name                     # the same stop step
        live = ref_score > -5e6
        assert torch.equal(seq.cpu()[live], ref_seq[live]), name
        assert bool((score.cpu()[~live] <= -5e6).all()), name
        rel = ((score.cpu()[live].double() - ref_score[live].double()).abs() / ref_score[live].double().abs().clamp_min(1e-3))
        assert float(rel.max()) < 2e-5, name


def test_decode_is_deterministic_and_records_its_stop(dev):
    from multimodal import ops
    torch.manual_seed(0)
    te, lm = _lm(dev, True, V=V_SAYCAM, E=512)
    with torch.no_grad():
        for p in te.parameters():
            p.normal_(0, 0.05)
        lm.output_layer.bias.normal_(0, 0.5)
        feats = torch.randn(256, 512, device=dev)
        s1, p1 = lm.beam_search_decode(256, 3, 25, 0.6, image_features=feats)
        s2, p2 = lm.beam_search_decode(256, 3, 25, 0.6, image_features=feats)
        s0, _ = lm.beam_search_decode(256, 3, 25, 0.6)                          # zero state: a different decode
        # a strong <eos> bias: every item finishes on its first token and the device stop test ends the decode at step 1
        lm.output_layer.bias[3] += 40.0
        s3, p3, n3 = ops.beam_search_lstm(te.embedding.weight, te.lstm, lm.output_layer.weight, lm.output_layer.bias, 256, 3, 25,
                                          0.6, *te.initial_state(feats), return_steps=True)
    assert torch.equal(s1, s2) and torch.equal(p1, p2)
    assert s1.dtype == torch.int64 and s1.shape[:2] == (256, 3) and p1.shape == (256, 3)
    assert not torch.equal(s0[:, 0, :s1.shape[2]], s1[:, 0, :s0.shape[2]])
    assert n3 == 1 and tuple(s3.shape) == (256, 3, 2)
    assert bool((s3[:, 0] == torch.tensor([2, 3], device=dev)).all()) and bool((p3[:, 0] > -5e6).all())   # <sos> <eos>


def test_captioning_lstm_initial_state_matches_float64(dev):
    """ops.lstm_text with an initial state (the captioning encoder in eval) against nn.LSTM in float64, B = 256, L = 25."""
    from multimodal import ops
    torch.manual_seed(1)
    B, L, E, V = 256, 25, 512, V_SAYCAM
    lstm = torch.nn.LSTM(E, E)
    with torch.no_grad():
        for p in lstm.parameters():
            p.uniform_(-0.08, 0.08)
    table = torch.randn(V, E) * 0.5
    tok = torch.randint(4, V, (B, L))
    length = torch.randint(2, L + 1, (B,))
    length[0] = L
    h0, c0 = torch.randn(B, E) * 0.5, torch.randn(B, E) * 0.5
    ld = lstm.to(dev)
    with torch.no_grad():
        h, out = ops.lstm_text(table.to(dev), ld, tok.to(dev), length.to(dev), h0.to(dev), c0.to(dev))
        ref = torch.nn.LSTM(E, E).double()
        ref.load_state_dict({k: v.double().cpu() for k, v in lstm.state_dict().items()})
        x = table.double()[tok]
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, length, batch_first=True, enforce_sorted=False)
        o, (hn, cn) = ref(packed, (h0.double()[None], c0.double()[None]))
        o, _ = torch.nn.utils.rnn.pad_packed_sequence(o, batch_first=True)
    assert float((h.cpu().double() - hn[0]).abs().max()) < 2e-5
    assert float((out.cpu().double() - o).abs().max()) < 2e-5


def test_captioning_encoder_forward_uses_connector(dev):
    """TextEncoder(captioning).forward(image_features=...) = the LSTM from the connector's (h0, c0), in float64."""
    torch.manual_seed(2)
    te, lm = _lm(dev, True, V=60, E=32)
    with torch.no_grad():
        for p in te.parameters():
            p.normal_(0, 0.3)
        f = torch.randn(5, 32, device=dev)
        y = torch.randint(4, 60, (5, 9), device=dev)
        yl = torch.full((5,), 9, device=dev)
        ret, out, _ = te(y, yl, image_features=f)
        cw, cb = te.connector.weight.double().cpu(), te.connector.bias.double().cpu()
        st = f.double().cpu() @ cw.t() + cb
        ref = torch.nn.LSTM(32, 32).double()
        ref.load_state_dict({k: v.double().cpu() for k, v in te.lstm.state_dict().items()})
        o, (hn, _) = ref(te.embedding.weight.double().cpu()[y.cpu()].transpose(0, 1), (st[None, :, :32], st[None, :, 32:]))
        loss = lm.calculate_ce_loss(y, yl, image_features=f, tokenwise=True)[0]
    assert float((out.cpu().double() - o.transpose(0, 1)).abs().max()) < 1e-5
    assert float((ret.cpu().double() - hn[0]).abs().max()) < 1e-5
    assert loss.shape == (5, 8) and bool(torch.isfinite(loss).all())
