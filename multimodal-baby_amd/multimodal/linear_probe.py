"""Linear probe on the frozen DINO ResNeXt-50: the reference's linear_decoding.py / object_categories_linear_decoding.py (training)
and eval_linear_decoding.py / eval_object_categories_linear_decoding.py (4-way trials), on the HIP trunk.

Training (linear_decoding.py:97-136, 139-218): the whole model stays in train mode, so every step normalises with the batch's
statistics AND updates the BatchNorm running statistics; ``validate`` runs once after the last epoch in eval mode on those
drifted statistics.  The fc runs through ``ops.linear_f32`` (ResNet.forward), the cross entropy through
``cvcl_token_ce_fwd/bwd``.  Evaluation (eval_linear_decoding.py:53-57, 89-91) never calls ``.eval()``: each trial is scored with
its own batch statistics -- here T trials per device pass through the grouped train-mode BatchNorm pass
(``ResNet.grouped_bn``), or one plain train-mode pass per trial with ``trial_batch = 1``."""
from __future__ import annotations

import math
import os
import random
import time

import numpy as np
import torch

from . import ops

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MODEL_NAME = "dino_sfp_resnext50"


# ---- data (torchvision.datasets.ImageFolder + ToTensor + Normalize, which the reference uses) -------------------------------
def find_classes(root):
    """torchvision's rule: the sorted names of the subdirectories of root"""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"no class folders under {root}")
    return classes, {c: i for i, c in enumerate(classes)}


def make_dataset(root, class_to_idx):
    """torchvision's rule: per class in index order, a sorted os.walk (followlinks) of its folder, files in sorted order, kept if
    their lower-cased name ends in an image extension"""
    out = []
    for cls in sorted(class_to_idx, key=class_to_idx.get):
        d = os.path.join(root, cls)
        for r, _, files in sorted(os.walk(d, followlinks=True)):
            for f in sorted(files):
                if f.lower().endswith(IMG_EXTENSIONS):
                    out.append((os.path.join(r, f), class_to_idx[cls]))
    return out


class ImageFolder(torch.utils.data.Dataset):
    """ImageFolder(root, transform=Compose([ToTensor(), Normalize(ImageNet)])).  Decoded frames are cached: the transform is
    deterministic, so a cached frame is the one a fresh decode would give."""

    def __init__(self, root, cache=True):
        self.root = root
        self.classes, self.class_to_idx = find_classes(root)
        self.samples = make_dataset(root, self.class_to_idx)
        self.targets = [t for _, t in self.samples]
        self._cache = {} if cache else None

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        if self._cache is not None and i in self._cache:
            return self._cache[i], self.targets[i]
        x = load_image(self.samples[i][0])
        if self._cache is not None:
            self._cache[i] = x
        return x, self.targets[i]


def load_image(path):
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f).convert("RGB")
    a = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0)    # ToTensor
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    return (a - mean) / std                                                                              # Normalize


def subset_indices(targets, n_classes, subset):
    """linear_decoding.py:67-76: per class random.sample(ceil(n * subset)), then one random.shuffle"""
    out = []
    for i in range(n_classes):
        idx = [j for j, x in enumerate(targets) if x == i]
        out += random.sample(idx, math.ceil(len(idx) * subset))
    random.shuffle(out)
    return out


def split_indices(targets, n_classes, split):
    """object_categories_linear_decoding.py:58-76: the first / last int(n * 0.5) of every class trains, the rest tests"""
    train, test = [], []
    for i in range(n_classes):
        idx = [j for j, x in enumerate(targets) if x == i]
        h = int(len(idx) * 0.5)
        a, b = (idx[:h], idx[h:]) if split == "first" else (idx[h:], idx[:h])
        train += a
        test += b
    return train, test


def build_loaders(args, variant, dataset_cls=None):
    """the reference's load_split_train_test, loader for loader (variant "saycam": --train_dir / --test_dir and --subset;
    "object_categories": one folder and --split).  dataset_cls (tests): a stand-in for ImageFolder taking the folder path."""
    dataset_cls = dataset_cls or ImageFolder
    kw = dict(batch_size=args.batch_size, num_workers=args.workers, pin_memory=False)
    train_data = dataset_cls(args.train_dir)
    if variant == "saycam":
        test_data = dataset_cls(args.test_dir)
        if args.subset == 1.0:
            train_loader = torch.utils.data.DataLoader(train_data, shuffle=True, **kw)
        else:
            idx = subset_indices(train_data.targets, len(train_data.classes), args.subset)
            train_loader = torch.utils.data.DataLoader(train_data, sampler=torch.utils.data.SubsetRandomSampler(idx), shuffle=False, **kw)
        test_loader = torch.utils.data.DataLoader(test_data, shuffle=False, **kw)
    else:
        test_data = dataset_cls(args.train_dir)
        tr, te = split_indices(train_data.targets, len(train_data.classes), args.split)
        train_loader = torch.utils.data.DataLoader(train_data, sampler=torch.utils.data.SubsetRandomSampler(tr), shuffle=False, **kw)
        test_loader = torch.utils.data.DataLoader(test_data, sampler=torch.utils.data.SubsetRandomSampler(te), shuffle=False, **kw)
    print("Total train data size is", len(train_loader) * args.batch_size)
    print("Total test data size is", len(test_loader) * args.batch_size)
    return train_loader, test_loader


# ---- meters (linear_decoding.py:221-276) -------------------------------------------------------------------------------------
class AverageMeter:
    """Computes and stores the average and current value"""

    def __init__(self, name, fmt=":f"):
        self.name = name
        self.fmt = fmt
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def __str__(self):
        fmtstr = "{name} {val" + self.fmt + "} ({avg" + self.fmt + "})"
        return fmtstr.format(**self.__dict__)


class ProgressMeter:
    def __init__(self, num_batches, meters, prefix=""):
        self.batch_fmtstr = self._get_batch_fmtstr(num_batches)
        self.meters = meters
        self.prefix = prefix

    def line(self, batch):
        return "\t".join([self.prefix + self.batch_fmtstr.format(batch)] + [str(m) for m in self.meters])

    def display(self, batch):
        print(self.line(batch))

    @staticmethod
    def _get_batch_fmtstr(num_batches):
        fmt = "{:" + str(len(str(num_batches // 1))) + "d}"
        return "[" + fmt + "/" + fmt.format(num_batches) + "]"


def accuracy(output, target, topk=(1,)):
    """percentage of rows whose target is among the k largest outputs (ties broken as torch.topk breaks them)"""
    with torch.no_grad():
        maxk = max(topk)
        batch_size = target.size(0)
        _, pred = output.topk(maxk, 1, True, True)
        correct = pred.t().eq(target.contiguous().view(1, -1))
        return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / batch_size) for k in topk]


# ---- model ---------------------------------------------------------------------------------------------------------------------
PRECISIONS = ("32", "bf16", "32-split")


def set_precision(model, precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r} not in {PRECISIONS}")
    model.compute_dtype = torch.bfloat16 if precision == "bf16" else torch.float32
    model.trunk_arithmetic = "split" if precision == "32-split" else "exact"


def build_probe(num_classes, random_init=False, precision="32", device="cuda"):
    """load_model("dino_sfp_resnext50"), trunk frozen, fc = Linear(2048, num_classes) (linear_decoding.py:97-103)"""
    from .utils import load_model
    model = load_model(MODEL_NAME, pretrained=not random_init)
    for p in model.parameters():
        p.requires_grad = False
    model.fc = torch.nn.Linear(in_features=2048, out_features=num_classes, bias=True)
    model = model.to(device)
    set_precision(model, precision)
    return model


def cross_entropy(output, target):
    """nn.CrossEntropyLoss() (mean over the batch) through the library's token cross-entropy kernels"""
    return ops.token_cross_entropy(output.contiguous(), target.long().contiguous(), -100).mean()


def train(train_loader, model, optimizer, epoch, args, device):
    """one epoch (linear_decoding.py:139-183): -> top-1 average as a numpy scalar"""
    batch_time = AverageMeter("Time", ":6.3f")
    data_time = AverageMeter("Data", ":6.3f")
    losses = AverageMeter("Loss", ":.4e")
    top1 = AverageMeter("Acc@1", ":6.2f")
    top5 = AverageMeter("Acc@5", ":6.2f")                  # (top-2, as the reference computes it)
    progress = ProgressMeter(len(train_loader), [batch_time, data_time, losses, top1, top5], prefix="Epoch: [{}]".format(epoch))
    model.train()
    end = time.time()
    for i, (images, target) in enumerate(train_loader):
        data_time.update(time.time() - end)
        images, target = images.to(device), target.to(device)
        output = model(images)
        loss = cross_entropy(output, target)
        acc1, acc5 = accuracy(output, target, topk=(1, 2))
        losses.update(loss.item(), images.size(0))
        top1.update(acc1[0], images.size(0))
        top5.update(acc5[0], images.size(0))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            progress.display(i)
    return top1.avg.cpu().numpy()


def validate(val_loader, model, device):
    """linear_decoding.py:186-218: eval mode; preds / target / images of the LAST batch"""
    batch_time = AverageMeter("Time", ":6.3f")
    top1 = AverageMeter("Acc@1", ":6.2f")
    model.eval()
    with torch.no_grad():
        end = time.time()
        for images, target in val_loader:
            images, target = images.to(device), target.to(device)
            output = model(images)
            preds = np.argmax(output.cpu().numpy(), axis=1)
            acc1 = accuracy(output, target, topk=(1,))
            top1.update(acc1[0].cpu().numpy()[0], images.size(0))
            batch_time.update(time.time() - end)
            end = time.time()
        print("* Acc@1 {top1.avg:.3f} ".format(top1=top1))
    return top1.avg, preds, target.cpu().numpy(), images.cpu().numpy()


def checkpoint_filename(args, variant):
    """linear_decoding.py:111, object_categories_linear_decoding.py:113"""
    if variant == "saycam":
        return f"self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_subset_{args.subset}_seed_{args.seed}.tar"
    return f"object_categories_self_supervised_dino_sfp_resnext50_labeled_s_linear_probe_seed_{args.seed}_split_{args.split}.tar"


def train_parser(variant):
    """the reference CLIs, flag for flag, plus --random_init, --precision and --out_dir"""
    import argparse
    p = argparse.ArgumentParser(description="Linear decoding with headcam data")
    p.add_argument("--train_dir", metavar="DIR", help="path to train dataset")
    if variant == "saycam":
        p.add_argument("--test_dir", metavar="DIR", help="path to test dataset")
    else:
        p.add_argument("--split", type=str, default="first", choices=["first", "last"], help="split to use for training")
    p.add_argument("-j", "--workers", default=8, type=int, metavar="N", help="number of data loading workers")
    p.add_argument("--epochs", default=100, type=int, metavar="N", help="number of total epochs to run")
    p.add_argument("--start-epoch", default=0, type=int, metavar="N", help="manual epoch number (useful on restarts)")
    p.add_argument("-b", "--batch-size", default=64, type=int, metavar="N", help="mini-batch size")
    p.add_argument("--lr", "--learning-rate", default=0.0005, type=float, metavar="LR", help="initial learning rate", dest="lr")
    p.add_argument("--wd", "--weight-decay", default=0.0, type=float, metavar="W", help="weight decay (default: 0)",
                   dest="weight_decay")
    p.add_argument("-p", "--print-freq", default=100, type=int, metavar="N", help="print frequency (default: 100)")
    p.add_argument("--num-classes", default=22 if variant == "saycam" else 64, type=int,
                   help="number of classes in downstream classification task")
    if variant == "saycam":
        p.add_argument("--subset", default=1.0, type=float, choices=[1.0, 0.1, 0.01],
                       help="proportion of training data to use for linear probe")
    p.add_argument("--seed", type=int, default=0, help="random seed")
    # additions of this implementation
    p.add_argument("--random_init", action="store_true", help="random-init trunk instead of the DINO weights")
    p.add_argument("--precision", type=str, default="32", choices=list(PRECISIONS), help="trunk arithmetic")
    p.add_argument("--out_dir", type=str, default="probe_results", help="where the .tar is written")
    return p


def train_main(args, variant):
    from .lightning import seed_everything
    device = torch.device("cuda:0")
    seed_everything(args.seed)
    model = build_probe(args.num_classes, args.random_init, args.precision, device)
    optimizer = torch.optim.Adam(model.parameters(), args.lr, weight_decay=args.weight_decay)
    os.makedirs(args.out_dir, exist_ok=True)
    savefile_name = os.path.join(args.out_dir, checkpoint_filename(args, variant))
    train_loader, test_loader = build_loaders(args, variant)
    acc1_list, val_acc1_list = [], []
    for epoch in range(args.start_epoch, args.epochs):
        acc1_list.append(train(train_loader, model, optimizer, epoch, args, device))
    val_acc1, preds, target, images = validate(test_loader, model, device)
    val_acc1_list.append(val_acc1)
    torch.save({"acc1_list": acc1_list, "val_acc1_list": val_acc1_list, "model_state_dict": model.state_dict(),
                "optimizer_state_dict": optimizer.state_dict(), "preds": preds, "target": target, "images": images},
               savefile_name)
    print(f"saved {savefile_name}")
    return savefile_name


# ---- evaluation (eval_linear_decoding.py, eval_object_categories_linear_decoding.py) ---------------------------------------
def eval_config(checkpoint, variant):
    """eval_linear_decoding.py:36-50 / eval_object_categories_linear_decoding.py:36-50"""
    config = {}
    if variant == "saycam":
        if "subset_0.1" in checkpoint:
            config["model"] = "embedding_linear_probe_10_percent"
        elif "subset_0.01" in checkpoint:
            config["model"] = "embedding_linear_probe_1_percent"
        else:
            config["model"] = "embedding_linear_probe"
    else:
        config["model"] = "embedding_object_categories_linear_probe"
    for s in (0, 1, 2):
        if f"seed_{s}" in checkpoint:
            config["seed"] = s
            break
    if variant != "saycam":
        if "split_first" in checkpoint:
            config["split"] = "first"
        elif "split_last" in checkpoint:
            config["split"] = "last"
    return config


def resolve_probe(checkpoint, root="probe_results"):
    return checkpoint if checkpoint.endswith(".tar") else os.path.join(root, f"{checkpoint}.tar")


def results_filename(config, variant):
    if variant == "saycam":
        return f"results/saycam/{config['model']}_seed_{config['seed']}_image_saycam_eval_predictions.json"
    return (f"results/object_categories/{config['model']}_seed_{config['seed']}_split_{config['split']}"
            "_image_object_categories_eval_predictions.json")


def load_probe(path, num_classes, precision, device):
    """resnext50_32x4d + fc(2048 -> num_classes), state dict loaded with strict=False; left in TRAIN mode, as the reference does"""
    from .resnext import resnext50_32x4d
    model = resnext50_32x4d()
    model.fc = torch.nn.Linear(in_features=2048, out_features=num_classes, bias=True)
    model = model.to(device)
    model.load_state_dict(torch.load(path, map_location=device, weights_only=False)["model_state_dict"], strict=False)
    for p in model.parameters():
        p.requires_grad = False
    set_precision(model, precision)
    return model


def score_trials(model, images, class_idx, group, trial_batch):
    """images [T * group, 3, H, W] (trial t = rows group t .. group t + group - 1), class_idx [T] -> (logits [T, group], pred [T]).
    trial_batch 1: one plain train-mode pass per trial (the reference's loop); else trial_batch trials per grouped pass."""
    T = images.shape[0] // group
    out = []
    with torch.no_grad():
        for t0 in range(0, T, max(trial_batch, 1)):
            t1 = min(T, t0 + max(trial_batch, 1))
            x = images[t0 * group:t1 * group]
            if trial_batch <= 1:
                o = model(x)
            else:
                with model.grouped_bn(group):
                    o = model(x)
            o = o.view(t1 - t0, group, -1)
            out.append(o[torch.arange(t1 - t0), :, class_idx[t0:t1]])
    logits = torch.cat(out)
    return logits, logits.argmax(dim=1)


def eval_parser(variant):
    import argparse
    p = argparse.ArgumentParser(description="Evaluation with linear probe models")
    p.add_argument("--checkpoint", type=str, help="path to linear probe checkpoint")
    p.add_argument("--save_predictions", action="store_true", help="save model predictions to JSON")
    # additions of this implementation
    p.add_argument("--eval_dataset", type=str, default=variant, choices=["saycam", "object_categories", "synthetic"],
                   help="evaluation trials (saycam / object_categories are private; synthetic: the synthetic data module's)")
    p.add_argument("--probe_root", type=str, default="probe_results", help="where checkpoint names resolve")
    p.add_argument("--trial_batch", type=int, default=64, help="trials per grouped pass (1 = the reference's loop)")
    p.add_argument("--precision", type=str, default="32", choices=list(PRECISIONS), help="trunk arithmetic")
    p.add_argument("--n_trials", type=int, default=32, help="number of synthetic trials")
    return p


def synthetic_trials(n_trials, device):
    """the synthetic evaluation trials of the data module eval.py uses: (images [T * 4, 3, H, W] fp32, class labels, metadata)"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    from train import _setup_parser
    from .multimodal_data_module import SyntheticDataModule
    data_args = _setup_parser().parse_args("")
    data_args.augment_frames = False
    data_args.eval_type = "image"
    data_args.n_eval_trials = n_trials
    data = SyntheticDataModule(data_args)
    data.prepare_data()
    data.setup()
    loader = data.test_dataloader()[1]
    meta = data.eval_sets["test"].metadata()
    imgs, labels = [], []
    for batch in loader:
        x = batch[0].squeeze(0).to(device)
        if x.dtype == torch.uint8:
            x = data.on_after_batch_transfer((x,), 1, training=False)[0]
        imgs.append(x.float())
        labels.append(batch[3][0][0])
    return torch.cat(imgs).contiguous(), labels, meta


def eval_main(args, variant):
    if args.eval_dataset != "synthetic":
        raise SystemExit(f"--eval_dataset {args.eval_dataset} reads the reference's private evaluation frames from hard-coded "
                         "cluster paths and is not available here; use --eval_dataset synthetic")
    device = torch.device("cuda:0")
    config = eval_config(args.checkpoint, variant)
    if variant != "saycam" and "split" not in config:
        raise SystemExit("object-category probes carry split_first / split_last in their name")
    num_classes = 22 if variant == "saycam" else 64
    path = resolve_probe(args.checkpoint, args.probe_root)
    fc_w = torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"].get("fc.weight")
    if fc_w is None or fc_w.shape[0] != num_classes:
        raise SystemExit(f"{path}: the probe's fc has {None if fc_w is None else fc_w.shape[0]} outputs, this evaluation expects "
                         f"{num_classes}")
    model = load_probe(path, num_classes, args.precision, device)
    images, labels, eval_data = synthetic_trials(args.n_trials, device)
    classes = sorted({t["target_category"] for t in eval_data})
    if len(classes) > num_classes:
        raise SystemExit(f"the synthetic evaluation has {len(classes)} categories, more than the probe's {num_classes} outputs")
    group = images.shape[0] // len(labels)
    class_idx = torch.tensor([classes.index(c) for c in labels], device=device)
    logits, preds = score_trials(model, images, class_idx, group, args.trial_batch)
    logits, preds = logits.cpu(), preds.cpu()
    correct_pred = {c: 0 for c in classes}
    total_pred = {c: 0 for c in classes}
    results = []
    for i, class_label in enumerate(labels):
        pred = int(preds[i])
        correct = pred == 0
        correct_pred[class_label] += int(correct)
        total_pred[class_label] += 1
        trial = eval_data[i]
        rec = {"checkpoint": args.checkpoint, "model": config["model"], "seed": config.get("seed"), "eval_type": "image",
               "eval_dataset": args.eval_dataset, "stage": "test", "trial_idx": i,
               "categories": [trial["target_category"]] + trial["foil_categories"], "logits": logits[i].tolist(), "pred": pred,
               "correct": correct}
        if variant != "saycam":
            rec["split"] = config["split"]
        results.append(rec)
    for classname, correct_count in correct_pred.items():
        if total_pred[classname]:
            print(f"Accuracy for class {classname:8s} is: {float(correct_count) / total_pred[classname]:.1%}")
    print(f"Total accuracy: {sum(correct_pred.values()) / sum(total_pred.values()):%}")
    if args.save_predictions:
        import json
        filename = results_filename(config, variant)
        os.makedirs(os.path.dirname(filename), exist_ok=True)
        print(f"Saving predictions to {filename}")
        with open(filename, "w") as f:
            json.dump({"data": results}, f)
    return results
