"""GPU: the captioning language model end to end -- the LSTM with an initial state and its backward (dh0, dc0), the captioning
cross entropy and its gradients against the reference (tests/golden/captioning_ce.npz), the Lightning wiring (LM-scored 4-way
trials, eval_textgen) and train.py --captioning."""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_lstm_initial_state_backward_matches_float64(dev):
    """LstmCore from (h0, c0) at B = 256, L = 25, H = 512: outputs, final h, dh0, dc0 and the weight gradients vs nn.LSTM in
    float64 over packed variable-length sequences."""
    from multimodal import text_train
    torch.manual_seed(3)
    B, L, E = 256, 25, 512
    lstm = torch.nn.LSTM(E, E)
    with torch.no_grad():
        for p in lstm.parameters():
            p.uniform_(-0.08, 0.08)
    x = torch.randn(B, L, E) * 0.5
    length = torch.randint(1, L + 1, (B,))
    length[0] = L
    h0, c0 = torch.randn(B, E) * 0.5, torch.randn(B, E) * 0.5
    r_out, r_h = torch.randn(B, L, E), torch.randn(B, E)
    r_out = r_out * (torch.arange(L)[None, :, None] < length[:, None, None])              # padded positions carry no loss

    ld = lstm.to(dev)
    xd = x.to(dev).reshape(B * L, E).requires_grad_(True)
    h0d, c0d = h0.to(dev).requires_grad_(True), c0.to(dev).requires_grad_(True)
    h, out = text_train.LstmCore.apply(xd, ld.weight_ih_l0, ld.weight_hh_l0, ld.bias_ih_l0, ld.bias_hh_l0, length.to(dev), B, L,
                                       h0d, c0d)
    ((out * r_out.to(dev)).sum() + (h * r_h.to(dev)).sum()).backward()

    ref = torch.nn.LSTM(E, E).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in lstm.state_dict().items()})
    xr = x.double().requires_grad_(True)
    h0r, c0r = h0.double().requires_grad_(True), c0.double().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xr, length, batch_first=True, enforce_sorted=False)
    o, (hn, _cn) = ref(packed, (h0r[None], c0r[None]))
    o, _ = torch.nn.utils.rnn.pad_packed_sequence(o, batch_first=True, total_length=L)
    ((o * r_out.double()).sum() + (hn[0] * r_h.double()).sum()).backward()

    def close(a, b, tol, what):
        a, b = a.detach().double().cpu(), b.detach().double()
        assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), what
    close(out, o, 2e-5, "out")
    close(h, hn[0], 2e-5, "h")
    close(h0d.grad, h0r.grad, 1e-4, "dh0")
    close(c0d.grad, c0r.grad, 1e-4, "dc0")
    close(xd.grad.view(B, L, E), xr.grad, 1e-4, "dx")
    for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        close(getattr(ld, name).grad, getattr(ref, name).grad, 1e-4, name)


def _caption_lm(dev, V, E, bias):
    import gen_golden_captioning as G
    from multimodal.multimodal import LanguageModel, TextEncoder
    vocab = {"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, **{f"w{i}": i for i in range(4, V)}}
    args = argparse.Namespace(text_encoder="lstm", embedding_type="flat", embedding_dim=E, crange=1, dropout_i=0.0, dropout_o=0.0,
                              pos_embed_type="no_pos_embed", captioning=True, attention=False, attention_gate=False, tie=True,
                              bias=True)
    with contextlib.redirect_stdout(io.StringIO()):
        te = TextEncoder(vocab, 2048, args)
        lm = LanguageModel(te, args)
    G.fill_text_encoder(te)
    with torch.no_grad():
        lm.output_layer.bias.copy_(bias)
    return te.to(dev).eval(), lm.to(dev).eval()


@pytest.mark.parametrize("case,V,E", [("toy", 50, 32), ("saycam", 2350, 512)])
def test_captioning_ce_loss_and_gradients_match_reference(dev, case, V, E):
    import gen_golden_captioning as G
    from multimodal import ops
    g = load_golden("captioning_ce")
    te, lm = _caption_lm(dev, V, E, G.ce_bias(V))
    y, yl = g[f"{case}.y"].to(dev), g[f"{case}.y_len"].to(dev)
    f = g[f"{case}.image_features"].to(dev).requires_grad_(True)
    loss, _o, logits, _a, labels = lm.calculate_ce_loss(y, yl, image_features=f, tokenwise=True)
    ref = g[f"{case}.loss"]
    Lp = ref.shape[1]
    assert torch.equal(labels.cpu()[:, :Lp], g[f"{case}.labels"])
    scale = max(1.0, float(logits.detach().abs().max()))
    assert float((loss.detach().cpu()[:, :Lp] - ref).abs().max()) < 5e-6 * scale
    means, _counts = ops.lm_loss_summaries(loss.reshape(-1), labels.reshape(-1))
    assert abs(float(means[0]) - float(g[f"{case}.mean"])) < 5e-6 * scale
    means[0].backward()

    def close(got, want, what):
        want = want.double()
        got = got.detach().double().cpu()[:want.shape[0]] if got.dim() > 1 and want.shape != got.shape else got.detach().double().cpu()
        assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max()) + 1e-7, what
    close(f.grad, g[f"{case}.d_image_features"], "d_image_features")
    close(lm.output_layer.bias.grad, g[f"{case}.d_out_bias"], "d_out_bias")
    params = dict(te.named_parameters())
    names = [k[len(case) + 3:] for k in g if k.startswith(f"{case}.g.")]
    assert {"connector.weight", "connector.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "embedding.weight"} <= set(names)
    for k in names:
        close(params[k].grad, g[f"{case}.g.{k}"], k)


def _lit_stub(dev, lm, encode):
    from multimodal.multimodal_lit import MultiModalLitModel
    lit = object.__new__(MultiModalLitModel)
    torch.nn.Module.__init__(lit)
    logged = {}
    lit.__dict__.update(lambda_mm=0.0, lambda_lm=1.0, optimize_unused=True, eval_textgen=True, beam_width=3, decode_length=25,
                        length_penalty_alpha=0.0, text_encoder=lm.text_encoder, training=False)
    lit.language_model = lm
    lit.model = types.SimpleNamespace(encode_image=encode, global_negatives=True)
    lit.log = lambda name, value, *a, **k: logged.__setitem__(name, value)
    return lit, logged


def test_lm_scored_trials_and_eval_textgen(dev):
    """Captioning with lambda_mm = 0: a 4-way trial is scored by the LM (logits = - the first token's cross entropy per image,
    reference multimodal_lit.py:478-495), and eval_textgen fills gen_text from the top beam of beam_search_decode."""
    import gen_golden_captioning as G
    torch.manual_seed(4)
    te, lm = _caption_lm(dev, 50, 32, G.output_bias(1.0))
    proj = torch.randn(3, 32, device=dev)
    encode = lambda x: (x.reshape(x.shape[0], -1)[:, :3] @ proj, None)       # a fixed "encoder": images -> flat features
    lit, logged = _lit_stub(dev, lm, encode)
    x = torch.randn(1, 4, 3, 8, 8, device=dev)
    y = torch.tensor([[2, 7, 3]], device=dev)
    yl = torch.tensor([3], device=dev)
    with torch.no_grad():
        ret = lit.validation_test_step("val", (x, y, yl, [["w7"]]), 0, dataloader_idx=1)
        feats = encode(x.view(4, 3, 8, 8))[0]
        ce = lm.calculate_ce_loss(y.expand(4, -1).contiguous(), yl.expand(4).contiguous(), image_features=feats, tokenwise=True)[0]
    want = -ce[:, 0]
    assert ret["accuracy"] == int(int(torch.argmax(want)) == 0)
    assert logged["val_accuracy"] == ret["accuracy"] and "val_entropy" in logged and "val_accuracy_w7" in logged
    # the same logits from float64 torch: connector state -> one LSTM step from <sos> -> log_softmax at token 7
    st = feats.double().cpu() @ te.connector.weight.double().cpu().t() + te.connector.bias.double().cpu()
    cell = torch.nn.LSTMCell(32, 32).double()
    cell.load_state_dict({k.replace("_l0", ""): v.double().cpu() for k, v in te.lstm.state_dict().items()})
    h, _ = cell(te.embedding.weight.double().cpu()[2].expand(4, -1), (st[:, :32], st[:, 32:]))
    lg = h @ te.embedding.weight.double().cpu().t() + lm.output_layer.bias.double().cpu()
    assert float((want.double().cpu() - lg.log_softmax(-1)[:, 7]).abs().max()) < 1e-5

    B = 6
    xb = torch.randn(B, 3, 8, 8, device=dev)
    yb = torch.tensor([[2, 5, 6, 3]] * B, device=dev)
    ylb = torch.full((B,), 4, device=dev)
    with torch.no_grad():
        out = lit.calculate_joint_loss((xb, yb, ylb, [f"ref {i}" for i in range(B)]), "val", lambda *a, **k: None, eval_textgen=True)
        seq, _ = lm.beam_search_decode(B, 3, 25, 0.0, image_features=encode(xb)[0])
    assert out["raw_y"] == [f"ref {i}" for i in range(B)] and len(out["gen_text"]) == B
    assert out["gen_text"] == [lit._ids_to_sentence(s) for s in seq[:, 0].tolist()]
    assert any(out["gen_text"]) and all(isinstance(t, str) for t in out["gen_text"])
    with contextlib.redirect_stdout(io.StringIO()) as so:
        lit.joint_loss_epoch_end([out], "val", lit.log, eval_textgen=True)
    assert "hypothesis:" in so.getvalue() and "val_ce_loss" in logged


def test_train_captioning_fast_dev_run(dev, tmp_path):
    """train.py --captioning trains end to end (lambda_lm 1, the connector's state feeding the LSTM) and runs eval_textgen."""
    code = ("import sys, torch; sys.path.insert(0, %r); import train; "
            "torch.manual_seed(0); trainer, lit = train.main(sys.argv[1:]); m = trainer.logged_metrics; "
            "assert trainer.global_step == 1 and 'train_ce_loss' in m and bool(torch.isfinite(torch.as_tensor(float(m['train_loss'])))); "
            "print('CAPTIONING_OK')") % ROOT
    argv = ("--dataset synthetic --batch_size=8 --gpus=1 --num_workers=2 --checkpoint_callback=False --logger=False "
            "--fast_dev_run --text_encoder lstm --lambda_mm 0 --lambda_lm 1 --captioning --eval_textgen --embedding_dim 64 "
            "--dropout_i 0").split()
    r = subprocess.run([sys.executable, "-c", code, *argv], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CAPTIONING_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
