"""CPU: the linear probe's host logic (multimodal/linear_probe.py) against the reference's own functions
(tests/golden/linear_probe.npz, tools/gen_golden_linear_probe.py) and torchvision's published ImageFolder rule."""
import argparse
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

from multimodal import linear_probe as L
from multimodal.lightning import seed_everything

G = load_golden("linear_probe")
LAYOUT = tuple(int(v) for v in G["layout"])
BATCH = int(G["batch"])


class LayoutFolder(torch.utils.data.Dataset):
    """the generator's ImageFolder stand-in: targets grouped by class, item = (index, target)"""

    def __init__(self, root):
        self.classes = [f"c{i}" for i in range(len(LAYOUT))]
        self.targets = [c for c, n in enumerate(LAYOUT) for _ in range(n)]

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return torch.tensor(i), self.targets[i]


def _epoch(loader):
    return np.concatenate([b[0].numpy() for b in loader])


def _loaders(variant, seed, **kw):
    args = argparse.Namespace(train_dir="train", test_dir="test", batch_size=BATCH, workers=0, **kw)
    seed_everything(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return L.build_loaders(args, variant, dataset_cls=LayoutFolder)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("subset", [1.0, 0.1, 0.01])
def test_subset_indices_and_batch_order_match_the_reference(seed, subset):
    tr, te = _loaders("saycam", seed, subset=subset)
    if subset != 1.0:
        assert list(tr.sampler.indices) == G[f"subset_{subset}_seed_{seed}_indices"].tolist()
    assert _epoch(tr).tolist() == G[f"subset_{subset}_seed_{seed}_epoch0"].tolist()
    assert _epoch(te).tolist() == list(range(sum(LAYOUT)))           # test loader: shuffle=False


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("split", ["first", "last"])
def test_split_indices_and_batch_order_match_the_reference(seed, split):
    tr, te = _loaders("object_categories", seed, split=split)
    assert list(tr.sampler.indices) == G[f"split_{split}_seed_{seed}_train_indices"].tolist()
    assert list(te.sampler.indices) == G[f"split_{split}_seed_{seed}_test_indices"].tolist()
    assert _epoch(tr).tolist() == G[f"split_{split}_seed_{seed}_epoch0"].tolist()
    assert _epoch(te).tolist() == G[f"split_{split}_seed_{seed}_test_epoch0"].tolist()


def test_accuracy_matches_the_reference():
    got = L.accuracy(G["acc_logits"], G["acc_target"], topk=(1, 2))
    assert [float(v) for v in got] == G["acc_top1_top2"].tolist()


def test_meter_strings_match_the_reference():
    m = [L.AverageMeter("Time", ":6.3f"), L.AverageMeter("Loss", ":.4e"), L.AverageMeter("Acc@1", ":6.2f")]
    for i, (v, n) in enumerate([(0.5, 16), (1.25, 16), (3.0, 7)]):
        for k, meter in enumerate(m):
            meter.update(v * (k + 1) + i, n)
    lines = [L.ProgressMeter(137, m, prefix="Epoch: [3]").line(42), L.ProgressMeter(9, m[:1], prefix="").line(0)]
    assert lines == G["meter_lines"].tolist()


def test_image_folder_follows_torchvision_rule(tmp_path):
    """classes = sorted sub-directories; per class a sorted os.walk, files sorted, only image extensions (case-insensitive)"""
    from PIL import Image
    layout = {"zebra": ["b.png", "a.JPG", "notes.txt", "sub/c.jpeg", "sub/deeper/d.bmp", "aa/e.ppm"],
              "Apple": ["x.png", "y.gif", ".hidden.png"], "mango": ["m.tiff"], "empty": []}
    for cls, files in layout.items():
        os.makedirs(tmp_path / cls, exist_ok=True)
        for f in files:
            p = tmp_path / cls / f
            os.makedirs(p.parent, exist_ok=True)
            if f.endswith((".txt", ".gif")):
                p.write_text("x")
            else:
                Image.new("RGB", (4, 3), (10, 200, 30)).save(p, format={"jpg": "JPEG", "jpeg": "JPEG", "tiff": "TIFF", "bmp": "BMP",
                                                                         "ppm": "PPM"}.get(f.rsplit(".", 1)[1].lower(), "PNG"))
    (tmp_path / "loose.png").write_text("not a class")
    ds = L.ImageFolder(str(tmp_path))
    assert ds.classes == ["Apple", "empty", "mango", "zebra"]
    rel = [(os.path.relpath(p, tmp_path), t) for p, t in ds.samples]
    assert rel == [("Apple/.hidden.png", 0), ("Apple/x.png", 0), ("mango/m.tiff", 2), ("zebra/a.JPG", 3), ("zebra/b.png", 3),
                   ("zebra/aa/e.ppm", 3), ("zebra/sub/c.jpeg", 3), ("zebra/sub/deeper/d.bmp", 3)]
    assert ds.targets == [t for _, t in rel]
    x, t = ds[4]
    assert t == 3 and x.shape == (3, 3, 4) and x.dtype == torch.float32
    want = (torch.tensor([10, 200, 30]) / 255.0 - torch.tensor(L.IMAGENET_MEAN)) / torch.tensor(L.IMAGENET_STD)
    assert torch.allclose(x[:, 0, 0], want.float(), atol=1e-6)


def test_file_names_and_checkpoint_config():
    a = argparse.Namespace(subset=0.1, seed=2, split="last")
    assert L.checkpoint_filename(a, "saycam") == "self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_subset_0.1_seed_2.tar"
    assert L.checkpoint_filename(a, "object_categories") == \
        "object_categories_self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_seed_2_split_last.tar"
    c = L.eval_config("self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_subset_0.01_seed_1", "saycam")
    assert c == {"model": "embedding_linear_probe_1_percent", "seed": 1}
    assert L.eval_config("x_subset_0.1_seed_0", "saycam")["model"] == "embedding_linear_probe_10_percent"
    assert L.eval_config("x_subset_1.0_seed_2", "saycam") == {"model": "embedding_linear_probe", "seed": 2}
    c = L.eval_config("object_categories_x_seed_0_split_first", "object_categories")
    assert c == {"model": "embedding_object_categories_linear_probe", "seed": 0, "split": "first"}
    assert L.results_filename({"model": "embedding_linear_probe", "seed": 0}, "saycam") == \
        "results/saycam/embedding_linear_probe_seed_0_image_saycam_eval_predictions.json"
    assert L.results_filename(c, "object_categories") == ("results/object_categories/embedding_object_categories_linear_probe_seed_0"
                                                          "_split_first_image_object_categories_eval_predictions.json")
    assert L.resolve_probe("name") == os.path.join("probe_results", "name.tar")
    assert L.resolve_probe("/a/b.tar", "elsewhere") == "/a/b.tar"


def test_reference_flags_parse():
    p = L.train_parser("saycam")
    a = p.parse_args(["--train_dir", "t", "--test_dir", "v", "--learning-rate", "0.01", "--wd", "0.1", "-b", "32", "--subset", "0.1",
                      "--num-classes", "5", "-j", "0", "--start-epoch", "1", "-p", "7"])
    assert (a.lr, a.weight_decay, a.batch_size, a.subset, a.num_classes, a.workers, a.start_epoch, a.print_freq) == \
        (0.01, 0.1, 32, 0.1, 5, 0, 1, 7)
    d = p.parse_args([])
    assert (d.lr, d.weight_decay, d.batch_size, d.subset, d.num_classes, d.epochs, d.seed, d.precision) == \
        (0.0005, 0.0, 64, 1.0, 22, 100, 0, "32")
    assert p.parse_args(["--lr", "0.2"]).lr == 0.2 and p.parse_args(["--weight-decay", "0.3"]).weight_decay == 0.3
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        p.parse_args(["--subset", "0.5"])
    q = L.train_parser("object_categories")
    b = q.parse_args(["--split", "last"])
    assert b.split == "last" and b.num_classes == 64 and not hasattr(b, "subset") and not hasattr(b, "test_dir")
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        q.parse_args(["--split", "middle"])
    e = L.eval_parser("saycam").parse_args(["--checkpoint", "c", "--save_predictions"])
    assert e.save_predictions and e.trial_batch == 64 and e.eval_dataset == "saycam"


def test_private_eval_datasets_exit():
    a = L.eval_parser("saycam").parse_args(["--checkpoint", "c"])
    with pytest.raises(SystemExit, match="synthetic"):
        L.eval_main(a, "saycam")
