"""GPU: ``eval.py --eval_dataset object_categories`` end to end on a small dataset on disk (tests/object_categories_common.py: 5
vocabulary folders + 1 that is no word, 3 JPEGs each of mixed sizes, a pattern per category) with (nearly) random-init checkpoints
written by train.py at --precision 32: the table path (every distinct frame and word encoded once, all 75 trials scored by one
``cvcl_trial_scores`` launch) against ``--no_trial_table --trial_batch 1``, the reference's loop through ``evaluate_trials``.

Tolerance between the two runs' probabilities.  It cannot be derived: the encoders' GEMM routes depend on the batch, so the features
of a frame encoded alone and in a batch differ in the last bits.  What batch composition alone does was MEASURED on the code without
the table path: the largest probability difference between ``eval.py --eval_dataset synthetic --trial_batch 64`` and
``--trial_batch 1`` (64 trials, both eval types) on this file's flat checkpoint,
    MEASURED = 4.470348e-07 on one MI355X (image 4.47e-07, text 2.98e-07; the spatial-mean checkpoint 2.98e-07 / 2.98e-07 and the
    CLIP-layout model 2.09e-07 / 3.87e-07 lie below it; no prediction differed),
and the table path, which changes the batch of BOTH encoders and not of one, is allowed 4 x that with a floor of 1e-6:
ALLOW = 1.788139e-06.  ``pred`` must agree wherever the per-trial run's top-two gap exceeds 2 ALLOW, and at least half the trials
must be decided that way -- otherwise the frames lack contrast and the comparison is vacuous.  (Seen when this was written: at most
3.6e-07 flat, 5.1e-07 with --use_kitty_label, 5.4e-07 spatial mean, 1.5e-07 CLIP layout; 75 of 75 trials decided in every run.)"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

import clip_common as CC
import object_categories_common as OC
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

SMALL = ("--batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --lambda_lm 0 --optimize_unused "
         "--normalize_features --logger False --num_workers 0")
EXP = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
RECORD_KEYS = ["checkpoint", "model", "seed", "shuffle_utterances", "augment_frames", "multiple_frames", "cnn", "eval_type", "eval_dataset",
               "stage", "trial_idx", "categories", "logits", "pred", "correct"]
MEASURED = 4.470348e-07                                  # largest |dp| of --trial_batch 64 vs 1 on synthetic trials, this checkpoint
ALLOW = max(4 * MEASURED, 1e-6)


def write_checkpoint(work, extra=""):
    """a (nearly) random-init checkpoint written by train.py on synthetic batches, as tests/test_frame_store_gpu.py writes its own"""
    import train
    cwd = os.getcwd()
    os.chdir(work)
    try:
        argv = f"--dataset synthetic {SMALL} --max_epochs 1 --limit_train_batches 1 --limit_val_batches 1 --checkpoint_callback True " \
               f"--exp_name {EXP} {extra}".split()
        with contextlib.redirect_stdout(io.StringIO()):
            train.main(argv)
    finally:
        os.chdir(cwd)
    return str(work)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return OC.materialize(tmp_path_factory.mktemp("objcat"))


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    return write_checkpoint(tmp_path_factory.mktemp("flat"))


@pytest.fixture(scope="module")
def spatial(tmp_path_factory):
    return write_checkpoint(tmp_path_factory.mktemp("spatial"), "--embedding_type spatial --sim mean")


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    from multimodal import clip_model as CM
    work = tmp_path_factory.mktemp("clip")
    bpe = CC.write_merges(work / "bpe.txt", CC.learn_merges(CC.vocab_words(), 300))
    sd = CC.random_state_dict(seed=26, W=128, layers=2, patch=32, R=224, Wt=128, tlayers=2, vocab=len(CM.SimpleTokenizer(bpe).encoder),
                              ctx=77, E=64, scale=2.0)
    torch.save(sd, work / "clip.pt")
    return str(work), ["--clip_eval", "--clip_checkpoint", str(work / "clip.pt"), "--clip_bpe", bpe]


def run_eval(work, model_args, dataset, eval_type, extra=()):
    """eval.py in ``work`` -> (returned records, the saved file's records)"""
    import eval as ev
    argv = list(model_args) + ["--eval_dataset", "object_categories", "--data_dir", dataset, "--eval_type", eval_type,
                               "--save_predictions"] + list(extra)
    args = ev._parser().parse_args(argv)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            results = ev.main(args)
        name = ev.clip_results_filename(args) if args.clip_eval else ev.results_filename(args, ev.config_from_checkpoint_name(EXP))
        assert name.startswith("results/object_categories/")
        with open(name) as f:
            saved = json.load(f)["data"]
    finally:
        os.chdir(cwd)
    return results, saved, out.getvalue()


def check_records(results, saved, printed, dataset, eval_type, classes=OC.CATEGORIES):
    with open(os.path.join(dataset, "eval_object_categories.json")) as f:
        trials = json.load(f)["data"]
    assert len(results) == len(trials) == 75 and saved == json.loads(json.dumps(results))
    totals = {}
    for i, (r, t) in enumerate(zip(results, trials)):
        assert list(r) == RECORD_KEYS and r["trial_idx"] == i and r["eval_type"] == eval_type
        assert r["eval_dataset"] == "object_categories" and r["stage"] == "test"
        assert r["categories"] == [t["target_category"]] + t["foil_categories"]
        p = np.array(r["logits"], dtype=np.float32)
        assert p.shape == (4,) and np.isfinite(p).all() and abs(float(p.sum()) - 1.0) < 1e-5
        assert r["pred"] == int(np.argmax(p)) and r["correct"] == (r["pred"] == 0)           # (numpy's arg-max is the lowest)
        totals[t["target_category"]] = totals.get(t["target_category"], 0) + 1
    assert totals == {c: 15 for c in OC.CATEGORIES}
    lines = [l for l in printed.splitlines() if l.startswith("Accuracy for class")]
    assert [l.split()[3] for l in lines] == list(classes)
    for c, l in zip(classes, lines):                       # 15 trials per class behind every printed share
        name = "cat" if c == "kitty" else c
        correct = sum(r["correct"] for r, t in zip(results, trials) if t["target_category"] == name)
        assert l.endswith(f"is: {correct / 15:.1%}")
    assert f"Total accuracy: {sum(r['correct'] for r in results) / 75:%}" in printed


def compare_runs(table, loop):
    """the table path's records against the per-trial loop's -> the largest probability difference"""
    pt, pl = (np.array([r["logits"] for r in rs], dtype=np.float64) for rs in (table, loop))
    diff = float(np.abs(pt - pl).max())
    print(f"largest probability difference table vs per-trial: {diff:.3e} (allowance {ALLOW:.3e})")
    assert diff <= ALLOW, diff
    top = -np.sort(-pl, axis=1)
    decided = (top[:, 0] - top[:, 1]) > 2 * ALLOW
    print(f"trials decided beyond twice the allowance: {int(decided.sum())} of {len(decided)}")
    assert decided.sum() * 2 >= len(decided), "vacuous: the frames need more contrast"
    assert all(a["pred"] == b["pred"] for a, b, d in zip(table, loop, decided) if d)
    return diff


LOOP = ("--no_trial_table", "--trial_batch", "1")


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_flat_checkpoint(dev, dataset, flat, eval_type):
    model = ["--checkpoint", EXP]
    table = run_eval(flat, model, dataset, eval_type)
    check_records(*table, dataset, eval_type)
    loop = run_eval(flat, model, dataset, eval_type, LOOP)
    check_records(*loop, dataset, eval_type)
    compare_runs(table[0], loop[0])
    # the encoder pass size of the table path (4 * --trial_batch frames) is not part of the result beyond the allowance
    small = run_eval(flat, model, dataset, eval_type, ("--trial_batch", "1"))
    compare_runs(small[0], loop[0])


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_kitty_label(dev, dataset, flat, eval_type):
    model = ["--checkpoint", EXP]
    classes = [c for c in OC.CATEGORIES if c != "cat"] + ["kitty"]
    plain = run_eval(flat, model, dataset, eval_type)[0]
    kitty = run_eval(flat, model, dataset, eval_type, ("--use_kitty_label",))
    check_records(*kitty, dataset, eval_type, classes)
    n_cat = 0
    for a, b in zip(plain, kitty[0]):
        if a["categories"][0] == "cat":                    # another word for the target: other probabilities
            n_cat += 1
            assert a["logits"] != b["logits"]
        else:                                              # ("cat" as a foil stays "cat")
            assert a["logits"] == b["logits"] and a["pred"] == b["pred"]
    assert n_cat == 15
    loop = run_eval(flat, model, dataset, eval_type, LOOP + ("--use_kitty_label",))
    check_records(*loop, dataset, eval_type, classes)
    compare_runs(kitty[0], loop[0])


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_spatial_mean_checkpoint(dev, dataset, spatial, eval_type):
    model = ["--checkpoint", EXP]
    table = run_eval(spatial, model, dataset, eval_type)
    check_records(*table, dataset, eval_type)
    loop = run_eval(spatial, model, dataset, eval_type, LOOP)
    compare_runs(table[0], loop[0])


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_clip_layout_model(dev, dataset, clip, eval_type):
    work, model = clip
    table = run_eval(work, model, dataset, eval_type)
    check_records(*table, dataset, eval_type)
    assert table[0][0]["model"] == "clip" and table[0][0]["checkpoint"] == "clip_vitl_14"
    loop = run_eval(work, model, dataset, eval_type, LOOP)
    check_records(*loop, dataset, eval_type)
    compare_runs(table[0], loop[0])


def test_item_layouts(dev, dataset, clip):
    """the datasets' items as the reference lays them out, frames on the device through the transform each dataset is documented with"""
    import argparse
    from multimodal.multimodal_data_module import EOS_TOKEN_ID, SOS_TOKEN_ID
    from multimodal.object_categories_data_module import ObjectCategoriesDataModule
    from multimodal.preprocess import DevicePreprocess
    from PIL import Image

    def module(**kw):
        dm = ObjectCategoriesDataModule(argparse.Namespace(data_dir=dataset, **kw))
        with contextlib.redirect_stdout(io.StringIO()):
            dm.prepare_data()
            dm.setup()
        return dm

    base = DevicePreprocess(224, "stretch")
    dm = module(eval_type="image", clip_eval=False)
    k = next(i for i, t in enumerate(dm.data) if Image.open(t["target_img_filename"]).size == (37, 53))      # a frame that is resized
    trial = dm.data[k]
    imgs, label, label_len, raw = dm.eval_dataset[k]
    assert imgs.shape == (4, 3, 224, 224) and imgs.is_cuda and imgs.dtype == torch.float32
    assert label.tolist() == [dm.vocab[trial["target_category"]]] and label_len == 1 and raw == [trial["target_category"]]
    files = [trial["target_img_filename"]] + trial["foil_img_filenames"]
    assert torch.equal(imgs, base([Image.open(f).convert("RGB") for f in files])) and torch.equal(imgs, dm.load_frames(files))
    batch = next(iter(dm.test_dataloader()))
    assert batch[0].shape == (1, 4, 3, 224, 224) and batch[1].shape == (1, 1) and batch[2].tolist() == [1] and batch[3] == [[dm.data[0]["target_category"]]]
    wrapped = module(eval_type="image", clip_eval=False, eval_include_sos_eos=True).eval_dataset[k]
    assert wrapped[1].tolist() == [SOS_TOKEN_ID, dm.vocab[trial["target_category"]], EOS_TOKEN_ID] and wrapped[2] == 3
    text = module(eval_type="text", clip_eval=False)
    img, labels, lens, raw = text.eval_dataset[k]
    assert img.shape == (1, 3, 224, 224) and torch.equal(img[0], imgs[0]) and raw == [trial["target_category"]]
    assert labels.tolist() == [[text.vocab[w]] for w in [trial["target_category"]] + trial["foil_categories"]] and lens == [1, 1, 1, 1]
    batch = next(iter(text.test_dataloader()))
    assert batch[0].shape == (1, 1, 3, 224, 224) and batch[1].shape == (1, 4, 1) and batch[2].tolist() == [[1, 1, 1, 1]]
    # --clip_eval: CLIP token rows; CLIP's transform for the image dataset, the base one for the text dataset (as the reference)
    from multimodal.clip_model import clip_preprocess, tokenize
    bpe = clip[1][-1]
    cimg = module(eval_type="image", clip_eval=True, clip_bpe=bpe).eval_dataset[k]
    assert cimg[1].shape == (1, 77) and cimg[2] == 1 and torch.equal(cimg[1], tokenize([trial["target_category"]], bpe))
    assert torch.equal(cimg[0], clip_preprocess()([Image.open(f).convert("RGB") for f in files])) and not torch.equal(cimg[0][0], imgs[0])
    ctext = module(eval_type="text", clip_eval=True, clip_bpe=bpe).eval_dataset[k]
    assert ctext[1].shape == (4, 77) and ctext[2] == [1, 1, 1, 1] and torch.equal(ctext[0][0], imgs[0])


def test_bench_tool_runs_at_toy_sizes(dev, capsys):
    """tools/bench_object_categories.py once, in-process: it runs, and its timed entries carry median, minimum and maximum"""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.append(tools)
    import importlib
    importlib.import_module("bench_object_categories").main(["--categories", "5", "--frames", "2", "--trial_batch", "4",
                                                             "--per_trial_trials", "8", "--dims", "37", "--repeats", "2", "--window-ms", "2"])
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    s = res["scorer"]["T5440_n4_D37"]
    for key in ("hip_us", "eager_us"):
        assert 0 < s["min_" + key] <= s[key] <= s["max_" + key]
    assert s["pred_equal"] >= 5400 and s["max_abs_dp_vs_eager"] < 1e-5            # (random rows: a near-tie may flip in fp32)
    e = res["end_to_end"]
    assert (e["categories"], e["files"], e["trials"], e["per_trial_trials_timed"]) == (5, 10, 50, 8)
    assert e["per_trial_trials_per_s"] > 0 and e["table_trials_per_s"] > 0 and e["pred_agree"].endswith("/8")


def test_table_path_is_taken_and_refused_where_it_has_no_form(dev, dataset, flat, monkeypatch):
    """the default run calls the table scorer and never the per-trial one; --no_trial_table the other way round; sim == "max" has no
    table form"""
    import eval as ev
    from multimodal import trials
    calls = []
    real_table, real_loop = trials.evaluate_trial_table, ev.evaluate_trials
    monkeypatch.setattr(trials, "evaluate_trial_table", lambda *a, **k: calls.append("table") or real_table(*a, **k))
    monkeypatch.setattr(ev, "evaluate_trials", lambda *a, **k: calls.append("loop") or real_loop(*a, **k))
    run_eval(flat, ["--checkpoint", EXP], dataset, "image")
    assert calls == ["table"]
    del calls[:]
    run_eval(flat, ["--checkpoint", EXP], dataset, "image", ("--no_trial_table", "--trial_batch", "25"))
    assert calls == ["loop"] * 3

    class Max:
        embedding_type, sim = "spatial", "max"
    assert "maximum over locations" in trials.table_route(Max()) and trials.table_route(type("Mean", (), {"embedding_type": "spatial", "sim": "mean"})()) is None
    with pytest.raises(Exception, match="maximum over locations"):
        trials.encode_words_once(Max(), torch.zeros(1, 1, dtype=torch.long), [1])
