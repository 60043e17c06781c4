"""Beam-search decoding throughput of the captioning LSTM language model (saycam_lm text settings: E = H = 512, V = 2350) on
flat image features of B images: the HIP decode (LanguageModel.beam_search_decode -> ops.beam_search_lstm) against an eager torch
composition of the reference algorithm on the same GPU (a yardstick only, defined here).

    python tools/bench_textgen.py [--batch 256] [--beam 3] [--decode-length 25] [--alpha 0.0] [--repeats 7] [--window-ms 200] [--no-eager]

Timed by tools/timing.py: ms per decode, median [min, max], the two decodes alternating; prints one JSON line.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

INF = 1e7


def eager_decode(lm, feats, K, T, alpha, sos=2, eos=3):
    """The reference algorithm (beam_search.py, stop_early) as plain torch ops with a host sync per step."""
    te = lm.text_encoder
    B = feats.shape[0]
    Hd = te.hidden_dim
    V = te.vocab_size
    st = torch.nn.functional.linear(feats, te.connector.weight, te.connector.bias)
    h = st[:, :Hd].repeat_interleave(K, 0)
    c = st[:, Hd:].repeat_interleave(K, 0)
    dev = feats.device
    alive_lp = torch.tensor([[0.] + [-float("inf")] * (K - 1)], device=dev).repeat(B, 1)
    alive_seq = torch.full((B, K, 1), sos, dtype=torch.long, device=dev)
    fin_seq = torch.zeros(B, K, 1, dtype=torch.long, device=dev)
    fin_sc = torch.full((B, K), -INF, device=dev)
    fin_fl = torch.zeros(B, K, dtype=torch.bool, device=dev)
    bpos = torch.arange(B, device=dev)[:, None]
    cell = torch.nn.LSTMCell(te.input_dim, Hd).to(dev)
    cell.load_state_dict({k.replace("_l0", ""): v for k, v in te.lstm.state_dict().items()})
    max_lp = ((5.0 + T) / 6.0) ** alpha
    i = 0
    while i < T and not bool((fin_sc.max(1).values > alive_lp[:, 0] / max_lp).all()):
        x = te.embedding(alive_seq[:, :, -1].reshape(-1))
        h, c = cell(x, (h, c))
        logits = lm.output_layer(h).view(B, K, V)
        lp = ((5.0 + i + 1) / 6.0) ** alpha
        scores = ((logits.log_softmax(-1) + alive_lp[:, :, None]) / lp).view(B, K * V)
        ts, ti = scores.topk(2 * K)
        tlp = ts * lp
        beam, tok = ti // V, ti % V
        tseq = torch.cat([alive_seq[bpos, beam], tok[:, :, None]], 2)
        tfin = tok == eos
        _, a = (ts + tfin.float() * -INF).topk(K)
        alive_seq, alive_lp = tseq[bpos, a], tlp[bpos, a]
        rows = (bpos * K + beam[bpos, a]).reshape(-1)
        h, c = h[rows], c[rows]
        fs = torch.cat([torch.cat([fin_seq, torch.zeros_like(fin_seq[:, :, :1])], 2), tseq], 1)
        fsc = torch.cat([fin_sc, ts + (1. - tfin.float()) * -INF], 1)
        ffl = torch.cat([fin_fl, tfin], 1)
        _, f = fsc.topk(K)
        fin_seq, fin_sc, fin_fl = fs[bpos, f], fsc[bpos, f], ffl[bpos, f]
        i += 1
    any_fin = fin_fl.any(1)
    return torch.where(any_fin[:, None, None], fin_seq, alive_seq), torch.where(any_fin[:, None], fin_sc, alive_lp)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--decode-length", type=int, default=25)
    ap.add_argument("--alpha", type=float, default=0.0)
    timing.add_arguments(ap)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args(argv)
    from multimodal.multimodal import LanguageModel, TextEncoder
    from multimodal import _hip as H
    dev = torch.device("cuda:0")
    vocab = {"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, **{f"w{i}": i for i in range(4, 2350)}}
    args = argparse.Namespace(text_encoder="lstm", embedding_type="flat", embedding_dim=512, crange=1, dropout_i=0.0, dropout_o=0.0,
                              pos_embed_type="no_pos_embed", captioning=True, attention=False, attention_gate=False, tie=True, bias=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(vocab, 2048, args)
        lm = LanguageModel(te, args)
    with torch.no_grad():
        for p in te.parameters():
            p.uniform_(-0.1, 0.1)
        lm.output_layer.bias.normal_(0, 0.5)
    te, lm = te.to(dev).eval(), lm.to(dev).eval()
    feats = torch.nn.functional.normalize(torch.randn(a.batch, 512, device=dev), dim=1)
    B, K, T = a.batch, a.beam, a.decode_length
    with torch.no_grad():
        sides = {"hip_ms_per_decode": lambda: lm.beam_search_decode(B, K, T, a.alpha, image_features=feats)}
        if not a.no_eager:
            sides["eager_ms_per_decode"] = lambda: eager_decode(lm, feats, K, T, a.alpha)
        t = timing.entries(timing.measure(sides, **timing.keywords(a)), digits=3)
        hip_ms = t["hip_ms_per_decode"]
        seq, lp = lm.beam_search_decode(B, K, T, a.alpha, image_features=feats)
        H.prof_enable(True)
        lm.beam_search_decode(B, K, T, a.alpha, image_features=feats)
        torch.cuda.synchronize()
        launches = sum(n for _ms, n in H.prof_collect().values())
        H.prof_enable(False)
        rec = {"metric": "textgen_decode", "batch": B, "beam": K, "decode_length": T, "alpha": a.alpha, "steps": int(seq.shape[2]) - 1,
               **t, "captions_per_s": round(B / hip_ms * 1e3, 1), "hip_launches_per_decode": launches}
        if not a.no_eager:
            es, elp = eager_decode(lm, feats, K, T, a.alpha)
            rec.update({"speedup": round(t["eager_ms_per_decode"] / hip_ms, 2),
                        "top_beam_agreement": float((es[:, 0] == seq[:, 0]).all(1).float().mean()) if es.shape == seq.shape else None})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
