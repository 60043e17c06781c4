"""Write tests/golden/linear_probe.npz from the reference's own linear-probe functions (CPU, build container only).

    python tools/gen_golden_linear_probe.py [--reference DIR]

The reference's linear_decoding.py and object_categories_linear_decoding.py are imported with stand-ins for the modules they
import but do not use here (torchvision, the model loader) and a seed_everything that seeds as Lightning does (random, numpy,
torch).  A stand-in ImageFolder gives a fixed synthetic class layout and returns each sample's index as its "image", so the
reference's load_split_train_test yields its sampled indices and its first epoch's batch order directly.  Recorded, for seeds 0
and 1: the subset indices at --subset 0.1 / 0.01, the first epoch's batches at 0.1 and 1.0, the --split first / last indices and
batches; accuracy() at top-(1, 2) on tie-free logits; AverageMeter / ProgressMeter strings.  Fixed zip timestamps: re-running
reproduces the archive byte for byte."""
import argparse
import importlib.util
import io
import os
import random
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "linear_probe.npz")
LAYOUT = (23, 7, 1, 40, 12, 3, 18, 9)         # images per class of the synthetic train folder
BATCH = 16


class LayoutFolder(torch.utils.data.Dataset):
    """ImageFolder stand-in: classes c0.., targets grouped by class in order (as ImageFolder lists them), item = (index, target)"""

    def __init__(self, root, transform=None):
        self.classes = [f"c{i}" for i in range(len(LAYOUT))]
        self.targets = [c for c, n in enumerate(LAYOUT) for _ in range(n)]

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return torch.tensor(i), self.targets[i]


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return seed


def load_reference(ref_dir, name):
    tv = types.ModuleType("torchvision")
    tv.transforms = types.SimpleNamespace(Normalize=lambda **k: None, Compose=lambda t: None, ToTensor=lambda: None)
    tv.datasets = types.SimpleNamespace(ImageFolder=LayoutFolder)
    tv.models = types.SimpleNamespace()
    pl = types.ModuleType("pytorch_lightning")
    pl.seed_everything = seed_everything
    mm = types.ModuleType("multimodal")
    mmu = types.ModuleType("multimodal.utils")
    mmu.load_model = lambda *a, **k: None
    mm.utils = mmu
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.datasets": tv.datasets,
                        "torchvision.models": tv.models, "pytorch_lightning": pl, "multimodal": mm, "multimodal.utils": mmu})
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_dir, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def first_epoch(loader):
    return np.concatenate([b[0].numpy() for b in loader]).astype(np.int64)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CVCL_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    ld = load_reference(a.reference, "linear_decoding")
    oc = load_reference(a.reference, "object_categories_linear_decoding")
    out = {"layout": np.array(LAYOUT, dtype=np.int64), "batch": np.array(BATCH)}
    for seed in (0, 1):
        for subset in (1.0, 0.1, 0.01):
            args = argparse.Namespace(subset=subset, batch_size=BATCH, workers=0)
            seed_everything(seed)
            tr, _ = ld.load_split_train_test("train", "test", args)
            if subset != 1.0:
                out[f"subset_{subset}_seed_{seed}_indices"] = np.array(tr.sampler.indices, dtype=np.int64)
            out[f"subset_{subset}_seed_{seed}_epoch0"] = first_epoch(tr)
        for split in ("first", "last"):
            args = argparse.Namespace(split=split, batch_size=BATCH, workers=0)
            seed_everything(seed)
            tr, te = oc.load_split_train_test("train", args)
            out[f"split_{split}_seed_{seed}_train_indices"] = np.array(tr.sampler.indices, dtype=np.int64)
            out[f"split_{split}_seed_{seed}_test_indices"] = np.array(te.sampler.indices, dtype=np.int64)
            out[f"split_{split}_seed_{seed}_epoch0"] = first_epoch(tr)
            out[f"split_{split}_seed_{seed}_test_epoch0"] = first_epoch(te)
    # accuracy at top-(1, 2) on tie-free logits (a permutation of distinct values per row)
    g = torch.Generator().manual_seed(5)
    logits = torch.stack([torch.randperm(22, generator=g).float() * 0.37 - 3.0 for _ in range(50)])
    target = torch.randint(0, 22, (50,), generator=g)
    target[:10] = logits[:10].argmax(1)
    target[10:20] = logits[10:20].topk(2, 1).indices[:, 1]
    out["acc_logits"], out["acc_target"] = logits.numpy(), target.numpy()
    out["acc_top1_top2"] = np.array([float(v) for v in ld.accuracy(logits, target, topk=(1, 2))], dtype=np.float64)
    # meters
    m = [ld.AverageMeter("Time", ":6.3f"), ld.AverageMeter("Loss", ":.4e"), ld.AverageMeter("Acc@1", ":6.2f")]
    for i, (v, n) in enumerate([(0.5, 16), (1.25, 16), (3.0, 7)]):
        for k, meter in enumerate(m):
            meter.update(v * (k + 1) + i, n)
    buf = io.StringIO()
    old, sys.stdout = sys.stdout, buf
    try:
        ld.ProgressMeter(137, m, prefix="Epoch: [3]").display(42)
        ld.ProgressMeter(9, m[:1], prefix="").display(0)
    finally:
        sys.stdout = old
    out["meter_lines"] = np.array(buf.getvalue().splitlines())
    write_npz(OUT, out)
    print(f"wrote {OUT}: {len(out)} arrays")


if __name__ == "__main__":
    main()
