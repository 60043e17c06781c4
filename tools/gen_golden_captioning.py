"""Generate tests/golden/captioning_beam.npz from the reference's own LanguageModel.beam_search_decode, run on the CPU.

    python tools/gen_golden_captioning.py [REFERENCE_CHECKOUT]

Small LSTM language models (V = 50, E = H = 32), plain (zero initial state) and captioning (the connector's state of flat image
features), decoded with beam widths 1, 3 and 5, alpha 0 and 0.6, decode lengths 10 and 25, and three output biases on <eos>: a
mild one (some items finish, some do not), a middle one (items finish at different steps; the stop test ends most decodes after
several steps) and a strong one (every item finishes at once).  Weights are formula-filled (oracle/gen_golden.formula_fill_,
tag = index of the sorted state_dict key) and rebuilt by the test, so the file holds inputs and outputs only.  Every kept case is robust: re-decoded with +-1e-4 uniform noise
on the logits it yields the same tokens and length, so fp32 summation order cannot flip a choice.  The archive is written with
fixed zip timestamps: re-running reproduces it byte for byte.

Captioning cross-entropy cases (tests/golden/captioning_ce.npz): the reference's LanguageModel.calculate_ce_loss with
image_features, tokenwise, and the gradients of the mean loss wrt the connector, the LSTM, the tied table, the output bias and the
image features; at toy size (B = 6, L = 9, V = 50, E = 32) in full, and at saycam_lm size (B = 16, L = 25, V = 2350, E = 512,
dropout_i 0) with the weight matrices' gradients reduced to their first 8 rows.
"""
import argparse
import contextlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402

V, E, B = 50, 32, 6
EOS_BIAS = {"mild": 0.5, "mid": 1.0, "strong": 4.0}
WEIGHT_SCALE = {"embedding.weight": 0.8, "connector.weight": 0.6, "connector.bias": 0.4}


def fill_text_encoder(te):
    """The formula fill the test rebuilds (tests/test_captioning_gpu.py)."""
    sd = te.state_dict()
    for i, k in enumerate(sorted(sd)):
        gen_golden.formula_fill_(sd[k], i, WEIGHT_SCALE.get(k, 0.5))


def output_bias(eos_bias):
    b = torch.empty(V)
    gen_golden.formula_fill_(b, 99, 0.5)
    b[3] += eos_bias
    return b


def build(mm, captioning, V=V, E=E):
    args = gen_golden.text_args("lstm", E)
    args.dropout_i = 0.0
    args.captioning = captioning
    with contextlib.redirect_stdout(io.StringIO()):
        te = mm.TextEncoder(gen_golden.small_vocab(V), 2048, args).eval()
        lm = mm.LanguageModel(te, argparse.Namespace(tie=True, bias=True)).eval()
    fill_text_encoder(te)
    return te, lm


class Noisy(torch.nn.Module):
    def __init__(self, lin, seed):
        super().__init__()
        self.lin, self.g = lin, torch.Generator().manual_seed(seed)

    def forward(self, x):
        y = self.lin(x)
        return y + (torch.rand(y.shape, generator=self.g, dtype=y.dtype) * 2 - 1) * 1e-4


def decode(lm, K, T, alpha, feats):
    with torch.no_grad():
        return lm.beam_search_decode(B, K, T, alpha, image_features=feats)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def ce_tokens(B, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(4, V, (B, L), generator=g)
    y_len = torch.randint(3, L + 1, (B,), generator=g)
    y_len[0] = L
    y[:, 0] = 2
    for b in range(B):
        y[b, int(y_len[b]) - 1] = 3
        y[b, int(y_len[b]):] = 0
    return y, y_len


def ce_bias(V):
    b = torch.empty(V)
    gen_golden.formula_fill_(b, 98, 0.5)
    return b


def ce_case(mm, name, B, L, V, E, full):
    te, lm = build(mm, True, V=V, E=E)
    with torch.no_grad():
        lm.output_layer.bias.copy_(ce_bias(V))
    y, y_len = ce_tokens(B, L, V, seed=B + L)
    feats = (torch.randn(B, E, generator=torch.Generator().manual_seed(L)) * 0.5).requires_grad_(True)
    loss, _o, _lg, _a, labels = lm.calculate_ce_loss(y, y_len, image_features=feats, tokenwise=True)
    mean = loss.sum() / (labels != 0).sum()
    mean.backward()
    out = {f"{name}.y": y.numpy(), f"{name}.y_len": y_len.numpy(), f"{name}.image_features": feats.detach().numpy(),
           f"{name}.loss": loss.detach().numpy(), f"{name}.labels": labels.numpy(), f"{name}.mean": mean.detach().numpy(),
           f"{name}.d_image_features": feats.grad.numpy(), f"{name}.d_out_bias": lm.output_layer.bias.grad.numpy()}
    for k, p in te.named_parameters():
        if p.grad is not None:
            out[f"{name}.g.{k}"] = (p.grad if full or p.grad.dim() == 1 else p.grad[:8]).numpy()
    return out


def main():
    if len(sys.argv) > 1:
        gen_golden.REF = sys.argv[1]
    gen_golden.install_stubs()
    from multimodal import multimodal as mm
    torch.set_num_threads(4)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, E, generator=g) * 2.0
    out = {"image_features": feats.numpy()}
    kept, dropped, early = 0, 0, 0
    for captioning in (False, True):
        te, lm = build(mm, captioning)
        if captioning:
            out["state_dict_keys"] = np.array(sorted(te.state_dict()))
        for bias_name, eb in EOS_BIAS.items():
            with torch.no_grad():
                lm.output_layer.bias.copy_(output_bias(eb))
            for K in (1, 3, 5):
                for alpha in (0.0, 0.6):
                    for T in (10, 25):
                        f = feats if captioning else None
                        seq, lp = decode(lm, K, T, alpha, f)
                        lin = lm.output_layer
                        robust = True
                        for seed in (1, 2):
                            lm.output_layer = Noisy(lin, seed)
                            try:
                                s2, _ = decode(lm, K, T, alpha, f)
                            finally:
                                lm.output_layer = lin
                            robust &= s2.shape == seq.shape and torch.equal(s2, seq)
                        name = f"{'cap' if captioning else 'plain'}_{bias_name}_k{K}_a{alpha}_t{T}"
                        if not robust:
                            dropped += 1
                            print(f"  {name}: not robust to 1e-4 logit noise, dropped")
                            continue
                        kept += 1
                        early += seq.shape[2] < T + 1
                        out[f"{name}.seq"] = seq.long().numpy()
                        out[f"{name}.score"] = lp.float().numpy()
    out["cases"] = np.array(sorted(k[:-4] for k in out if k.endswith(".seq")))
    ce = {}
    ce.update(ce_case(mm, "toy", 6, 9, V, E, True))
    ce.update(ce_case(mm, "saycam", 16, 25, 2350, 512, False))
    ce_path = os.path.join(ROOT, "tests", "golden", "captioning_ce.npz")
    write_npz(ce_path, ce)
    print(f"wrote {ce_path} ({os.path.getsize(ce_path) / 1024:.1f} KiB)")
    path = os.path.join(ROOT, "tests", "golden", "captioning_beam.npz")
    write_npz(path, out)
    print(f"kept {kept} cases ({early} stopped early), dropped {dropped}; wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
