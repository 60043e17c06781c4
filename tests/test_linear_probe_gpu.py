"""GPU: linear-probe training and evaluation (multimodal/linear_probe.py and the four top-level scripts).

Training steps are checked against a float64 restatement of the reference's step: the oracle trunk in train mode (batch
statistics, running-statistics EMA), then a torch float64 fc, cross entropy and Adam over the fc.  The scripts run end to end on
a small generated ImageFolder with a random-init trunk, and the evaluation gives the same decisions and logits whether trials are
scored one plain pass at a time (--trial_batch 1, the reference's loop) or in grouped passes (--trial_batch 64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cvcl_oracle as O
from conftest import ROOT, maxrel

pytestmark = pytest.mark.gpu

LR = 5e-4


def _probe(dev, n_classes=22, seed=0):
    from multimodal import linear_probe as L
    torch.manual_seed(seed)
    return L.build_probe(n_classes, random_init=True, precision="32", device=dev)


def _trunk_params(model):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in model.state_dict().items() if not k.startswith("fc.")}


@pytest.mark.parametrize("B,S,steps", [(16, 224, 3), (64, 64, 1)])
def test_probe_steps_vs_float64(dev, B, S, steps):
    """losses, top-1/top-2, fc weight and bias after Adam, all 53 layers' running statistics and num_batches_tracked, then
    validate() on the drifted statistics.  Adam moves every fc element by about lr whatever its gradient's size, so an element
    whose float64 gradient is within rounding of zero may move the other way: the fc check allows that for a few elements
    (at most 2 lr per step) and holds the rest to 1e-3 of the update."""
    from multimodal import linear_probe as L
    model = _probe(dev)
    opt = torch.optim.Adam(model.parameters(), LR, weight_decay=0.0)
    pd = _trunk_params(model)
    W = model.fc.weight.detach().cpu().double().clone().requires_grad_(True)
    b = model.fc.bias.detach().cpu().double().clone().requires_grad_(True)
    opt_ref = torch.optim.Adam([W, b], LR, weight_decay=0.0)
    g = torch.Generator().manual_seed(B + S)
    model.train()
    for step in range(steps):
        x = torch.randn(B, 3, S, S, generator=g)
        y = torch.randint(0, 22, (B,), generator=g)
        out = model(x.to(dev))
        loss = L.cross_entropy(out, y.to(dev))
        a1, a2 = L.accuracy(out, y.to(dev), topk=(1, 2))
        opt.zero_grad()
        loss.backward()
        opt.step()
        so = {}
        with torch.no_grad():
            pooled, _ = O.resnext50_forward(pd, x.double(), True, stats_out=so)
        pd.update(so)
        logits = pooled @ W.t() + b
        loss_ref = F.cross_entropy(logits, y)
        r1, r2 = L.accuracy(logits.detach(), y, topk=(1, 2))
        opt_ref.zero_grad()
        loss_ref.backward()
        opt_ref.step()
        print(f"B={B} {S}^2 step {step}: loss {float(loss):.6f} vs float64 {float(loss_ref):.6f}; logits rel "
              f"{maxrel(out, logits):.2e}")
        assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref)))
        assert maxrel(out, logits) < 2e-4
        assert (float(a1), float(a2)) == (float(r1), float(r2))
    torch.cuda.synchronize()
    for name, got, want in (("fc.weight", model.fc.weight, W), ("fc.bias", model.fc.bias, b)):
        err = (got.detach().cpu().double() - want.detach()).abs()
        assert float(err.max()) <= 2 * LR * steps + 1e-7, name
        assert float((err > 1e-3 * LR * steps).double().mean()) < 2e-3, name
    sd = model.state_dict()
    n_bn = 0
    for k, v in pd.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            n_bn += 1
            assert maxrel(sd[k], v) < 1e-4, k
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == steps, k
    assert n_bn == 2 * 53
    # validate(): eval mode on the drifted running statistics, preds / target / images of the last batch
    xv = torch.randn(2 * B, 3, S, S, generator=g)
    yv = torch.randint(0, 22, (2 * B,), generator=g)
    loader = [(xv[:B], yv[:B]), (xv[B:], yv[B:])]
    acc, preds, target, images = L.validate(loader, model, dev)
    with torch.no_grad():
        pooled_v, _ = O.resnext50_forward(pd, xv[B:].double(), False)
        lv = pooled_v @ W.detach().t() + b.detach()
    assert model.training is False
    assert np.array_equal(target, yv[B:].numpy()) and np.allclose(images, xv[B:].numpy())
    assert np.array_equal(preds, lv.argmax(1).numpy())


def _image_tree(root, n_classes, per_class, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for c in range(n_classes):
        d = os.path.join(root, f"class_{c:02d}")
        os.makedirs(d, exist_ok=True)
        for i in range(per_class):
            a = (rng.random((size, size, 3)) * 255).astype(np.uint8)
            a[..., c % 3] = np.clip(a[..., c % 3].astype(int) + 40 * (c % 5), 0, 255)
            Image.fromarray(a).save(os.path.join(d, f"img_{i:03d}.png"))


def _run(args, cwd, timeout=600):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_scripts_end_to_end(tmp_path):
    train_dir, test_dir = tmp_path / "train", tmp_path / "test"
    _image_tree(str(train_dir), 22, 10, 64, 1)
    _image_tree(str(test_dir), 22, 2, 64, 2)
    out = tmp_path / "probes"
    keys = {"acc1_list", "val_acc1_list", "model_state_dict", "optimizer_state_dict", "preds", "target", "images"}
    want_sd = set(O.resnext50_random_params(seed=0)) | {"fc.weight", "fc.bias"}
    s = _run([os.path.join(ROOT, "linear_decoding.py"), "--train_dir", str(train_dir), "--test_dir", str(test_dir), "--random_init",
              "--epochs", "2", "-b", "8", "--subset", "0.1", "-j", "0", "--out_dir", str(out)], tmp_path)
    assert "Epoch: [1]" in s and "* Acc@1" in s
    ck = out / "self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_subset_0.1_seed_0.tar"
    d = torch.load(ck, weights_only=False)
    assert set(d) == keys and len(d["acc1_list"]) == 2 and len(d["val_acc1_list"]) == 1
    assert set(d["model_state_dict"]) == want_sd
    assert d["model_state_dict"]["fc.weight"].shape == (22, 2048)
    assert int(d["model_state_dict"]["bn1.num_batches_tracked"]) == 2 * 3          # ceil(10 * 0.1) per class = 22 images, b 8
    # Adam over ALL parameters (linear_decoding.py:107): 53 convolutions, 53 BatchNorm weight / bias pairs, fc weight and bias
    assert len(d["optimizer_state_dict"]["param_groups"][0]["params"]) == 53 + 2 * 53 + 2
    _run([os.path.join(ROOT, "object_categories_linear_decoding.py"), "--train_dir", str(train_dir), "--random_init", "--epochs", "2",
          "-b", "16", "--split", "last", "--num-classes", "64", "-j", "0", "--out_dir", str(out)], tmp_path)
    ck2 = out / "object_categories_self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_seed_0_split_last.tar"
    d2 = torch.load(ck2, weights_only=False)
    assert set(d2) == keys and set(d2["model_state_dict"]) == want_sd
    assert d2["model_state_dict"]["fc.weight"].shape == (64, 2048)
    # evaluation: reference records, --trial_batch 1 (plain pass per trial) vs 64 (grouped passes)
    recs = {}
    for tb in (1, 64):
        wd = tmp_path / f"eval_{tb}"
        os.makedirs(wd)
        _run([os.path.join(ROOT, "eval_linear_decoding.py"), "--checkpoint", str(ck), "--eval_dataset", "synthetic",
              "--save_predictions", "--trial_batch", str(tb), "--n_trials", "16"], wd)
        f = wd / "results" / "saycam" / "embedding_linear_probe_10_percent_seed_0_image_saycam_eval_predictions.json"
        recs[tb] = json.load(open(f))["data"]
    assert len(recs[1]) == len(recs[64]) == 16
    fields = {"checkpoint", "model", "seed", "eval_type", "eval_dataset", "stage", "trial_idx", "categories", "logits", "pred",
              "correct"}
    for a, b in zip(recs[1], recs[64]):
        assert set(a) == fields
        assert a["pred"] == b["pred"] and a["correct"] == (a["pred"] == 0)
        assert maxrel(torch.tensor(b["logits"]), torch.tensor(a["logits"])) < 2e-4
    wd = tmp_path / "eval_oc"
    os.makedirs(wd)
    _run([os.path.join(ROOT, "eval_object_categories_linear_decoding.py"), "--checkpoint", str(ck2), "--eval_dataset", "synthetic",
          "--save_predictions", "--n_trials", "8"], wd)
    f = wd / "results" / "object_categories" / ("embedding_object_categories_linear_probe_seed_0_split_last"
                                               "_image_object_categories_eval_predictions.json")
    assert json.load(open(f))["data"][0]["split"] == "last"
    # a probe whose fc width does not match the evaluation is refused with a clear message
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_linear_decoding.py"), "--checkpoint", str(ck2), "--eval_dataset",
                        "synthetic"], cwd=wd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "outputs" in r.stderr
