"""GPU: the OpenAI-layout CLIP of multimodal/clip_model.py against the float64 restatement of tests/clip_common.py (itself pinned to
``transformers.CLIPModel`` in tests/test_clip_host.py), and ``eval.py --clip_eval`` end to end (reference eval.py:29-45, 205-207,
224-226, 287-288)."""
import json

import pytest
import torch
import torch.nn.functional as F

import clip_common as CC
from conftest import maxrel

pytestmark = pytest.mark.gpu

RECORD_KEYS = ["checkpoint", "model", "seed", "shuffle_utterances", "augment_frames", "multiple_frames", "cnn", "eval_type", "eval_dataset",
               "stage", "trial_idx", "categories", "logits", "pred", "correct"]                  # reference eval.py:249-265


@pytest.fixture(scope="module")
def case():
    """Vision: W 128, 2 layers, patch 14, R 84 (T = 37: the bf16 attention takes the MFMA kernel); text: Wt 128, 2 layers, vocab 512,
    context 77; E 64; logit_scale 2.  The float64 reference is computed once."""
    sd = CC.random_state_dict(seed=0, W=128, layers=2, patch=14, R=84, Wt=128, tlayers=2, vocab=512, ctx=77, E=64, scale=2.0)
    g = torch.Generator().manual_seed(1)
    image = torch.randn(5, 3, 84, 84, generator=g)
    tok = torch.zeros(6, 77, dtype=torch.long)
    for b, n in enumerate((1, 2, 7, 30, 75, 3)):
        tok[b, 0], tok[b, n + 1] = 510, 511
        tok[b, 1:n + 1] = torch.randint(1, 510, (n,), generator=g)
    ref = {"img": CC.encode_image(sd, image), "txt": CC.encode_text(sd, tok)}
    ref["lpi"], ref["lpt"] = CC.logits(sd, image, tok)
    return sd, image, tok, ref


@pytest.fixture(scope="module")
def model(case, dev):
    from multimodal import clip_model as CM
    return CM.build_model(case[0]).to(dev)


def test_fp32_features_and_logits(case, model, dev):
    _, image, tok, ref = case
    model.set_precision("32")
    img, txt = model.encode_image(image.to(dev)), model.encode_text(tok.to(dev))
    lpi, lpt = model(image.to(dev), tok.to(dev))
    e_img, e_txt, e_lpi, e_lpt = maxrel(img, ref["img"]), maxrel(txt, ref["txt"]), maxrel(lpi, ref["lpi"]), maxrel(lpt, ref["lpt"])
    print(f"[clip fp32] image features {e_img:.2e}, text features {e_txt:.2e}, logits {e_lpi:.2e}")
    assert img.shape == (5, 64) and txt.shape == (6, 64) and lpi.shape == (5, 6) and lpt.shape == (6, 5)
    assert img.dtype == torch.float32 and txt.dtype == torch.float32
    assert e_img < 2e-5 and e_txt < 2e-5                     # the fp32 ViT bound of test_encoders_gpu.py
    assert e_lpi < 1e-4 and e_lpt < 1e-4
    assert torch.equal(lpi, model(image.to(dev), tok.to(dev))[0])


def test_bf16_image_tower(case, model, dev):
    """The deviation of the bf16 image features from float64 is at most 1.5 x that of the restatement with bf16-rounded weights and
    GEMM inputs (+ 1e-3; the margin covers accumulation order), cosine per row > 0.999.  The text tower stays fp32.
    Measured on an MI355X: DESIGN.md section 9 "CLIP evaluation"."""
    sd, image, tok, ref = case
    model.set_precision("bf16")
    try:
        img = model.encode_image(image.to(dev)).double().cpu()
        txt = model.encode_text(tok.to(dev))
    finally:
        model.set_precision("32")
    emu = CC.encode_image(sd, image, rnd=CC.bf16_round)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    r_hip, r_emu = rel(img, ref["img"]), rel(emu, ref["img"])
    cos = float(F.cosine_similarity(img, ref["img"], dim=1).min())
    print(f"[clip bf16] rel-L2 vs float64: HIP {r_hip:.3e}, bf16-rounded restatement {r_emu:.3e}; min cosine {cos:.6f}")
    assert torch.isfinite(img).all()
    assert r_hip <= 1.5 * r_emu + 1e-3
    assert cos > 0.999
    assert maxrel(txt, ref["txt"]) < 2e-5


# ---- eval.py --clip_eval ------------------------------------------------------------------------------------------------------------
E2E_SEED = 26                                            # chosen on the CPU: every trial's top-1 - top-2 margin >= 2e-2 in both eval types


def _e2e_state_dict(vocab):
    return CC.random_state_dict(seed=E2E_SEED, W=128, layers=2, patch=32, R=224, Wt=128, tlayers=2, vocab=vocab, ctx=77, E=64, scale=2.0)


def e2e_oracle(eval_type, bpe_path, n_trials=6):
    """The restatement over the synthetic CLIP trials -> per trial (the 4 logits in float64, soft-max, prediction)."""
    import argparse
    from multimodal import clip_model as CM
    from multimodal.multimodal_data_module import SyntheticDataModule
    data = SyntheticDataModule(argparse.Namespace(eval_type=eval_type, n_eval_trials=n_trials, seed=0, clip_eval=True, clip_bpe=bpe_path))
    data.setup()
    sd = _e2e_state_dict(len(CM.SimpleTokenizer(bpe_path).encoder))
    out = []
    trials = data.eval_sets["test"]
    for imgs, label, _len, _raw in (trials[i] for i in range(len(trials))):
        lpi, lpt = CC.logits(sd, imgs, label)
        row = lpt[0] if eval_type == "image" else lpi[0]
        out.append((row, torch.softmax(row, -1), int(row.argmax())))
    return sd, out


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_eval_clip_end_to_end(dev, tmp_path, monkeypatch, eval_type):
    import eval as ev
    bpe = CC.write_merges(tmp_path / "bpe.txt", CC.learn_merges(CC.vocab_words(), 300))
    sd, oracle = e2e_oracle(eval_type, bpe)
    for row, _, _ in oracle:                                 # rounding cannot flip a prediction
        top = row.sort(descending=True).values
        assert float(top[0] - top[1]) >= 1e-2, row
    torch.save(sd, tmp_path / "clip.pt")
    monkeypatch.chdir(tmp_path)
    args = ev._parser().parse_args(["--clip_eval", "--clip_checkpoint", str(tmp_path / "clip.pt"), "--clip_bpe", bpe, "--eval_dataset", "synthetic",
                                    "--eval_type", eval_type, "--n_trials", "6", "--trial_batch", "4", "--save_predictions", "--use_kitty_label"])
    results = ev.main(args)
    with open(tmp_path / "results" / "synthetic" / f"clip_{eval_type}_synthetic_test_eval_predictions.json") as f:
        saved = json.load(f)["data"]
    assert saved == json.loads(json.dumps(results)) and len(saved) == 6
    for i, (rec, (row, soft, pred)) in enumerate(zip(saved, oracle)):
        assert list(rec) == RECORD_KEYS
        assert (rec["model"], rec["cnn"], rec["checkpoint"], rec["seed"], rec["trial_idx"]) == ("clip", "clip", "clip_vitl_14", None, i)
        assert rec["eval_type"] == eval_type and rec["eval_dataset"] == "synthetic" and rec["stage"] == "test" and len(rec["categories"]) == 4
        assert rec["pred"] == pred and rec["correct"] == (pred == 0)
        assert float((torch.tensor(rec["logits"], dtype=torch.float64) - soft).abs().max()) < 1e-4
