"""GPU: cvcl_augment_frames_indexed and the frame store.  Every kernel test compares the indexed launch, bit for bit on both the
fp32 tensor and the uint8 image, against cvcl_augment_frames (the existing entry) on the same frames gathered into a contiguous
batch with index_select; then the data module's --frame_store path against its --device_frames path, and train.py / eval.py on a
tiny SAYCam-layout dataset on disk."""
import contextlib
import importlib
import io
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import saycam_common as SC
from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

SMALL = ("--batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --lambda_lm 0 --optimize_unused "
         "--normalize_features --logger False --num_workers 0")


def _store(frames):
    from multimodal.frame_store import FrameStore
    return FrameStore(frames, {})


def _random_params(n, H, W, seed):
    """crop boxes anywhere in the frame (row 0: the whole frame), blur on two rows of three, random flips"""
    from multimodal.augment import FrameParams
    rng = np.random.default_rng(seed)
    crop, sigma, flip = [], [], []
    for i in range(n):
        h, w = (H, W) if i == 0 else (int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1)))
        crop.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
        sigma.append(float(rng.uniform(0.1, 2.0)) if i % 3 else 0.0)            # rows 0, 3: no blur
        flip.append(int(rng.integers(0, 2)))
    return FrameParams(crop, sigma, flip)


def _both(store, index, aug, params):
    """(indexed launch, plain launch on the gathered frames): each (fp32 out, uint8 out)"""
    got = store.transform(index, aug, params, return_uint8=True)
    gathered = store.frames.index_select(0, index.to(store.device))
    want = aug(gathered, params, return_uint8=True)
    return got, want


@pytest.mark.parametrize("H,W", [(224, 224), (240, 320), (100, 75)])
def test_gather_matches_plain_entry(dev, H, W):
    from multimodal.augment import DeviceFrameAugment, FrameParams
    g = torch.Generator().manual_seed(H * 1000 + W)
    store = _store(torch.randint(0, 256, (7, H, W, 3), dtype=torch.uint8, generator=g).to(dev))
    index = torch.tensor([6, 0, 3, 3, 6], dtype=torch.int64)                    # first and last frame, repeats
    aug = DeviceFrameAugment()
    rnd = _random_params(5, H, W, seed=H + W)
    assert float(rnd.sigma[0]) == 0.0 and float(rnd.sigma[1]) > 0
    for params in (rnd, FrameParams.identity(5, H, W)):
        (out, out8), (want, want8) = _both(store, index, aug, params)
        assert out.shape == (5, 3, 224, 224) and out8.shape == (5, 224, 224, 3)
        assert torch.equal(out8, want8) and torch.equal(out, want)
    # the same frame through the same parameters gives the same rows wherever it sits in the batch
    same = FrameParams(rnd.crop[[1, 1, 1, 1, 1]], rnd.sigma[[1, 1, 1, 1, 1]], rnd.flip[[1, 1, 1, 1, 1]])
    out = store.transform(index, aug, same)
    assert torch.equal(out[0], out[4]) and torch.equal(out[2], out[3]) and not torch.equal(out[0], out[1])


def test_offsets_past_2_31_and_2_32_bytes(dev):
    """a 4.30 GB store: frame 14267 is the first wholly past 2^31 bytes, 28533 the first wholly past 2^32, 28539 the last; a
    32-bit byte offset anywhere reads a zero or a wrong frame"""
    from multimodal.augment import DeviceFrameAugment, FrameParams
    N, per = 28540, 224 * 224 * 3
    assert 14266 * per < 2 ** 31 <= 14267 * per and 28532 * per < 2 ** 32 <= 28533 * per and (N - 1) * per > 2 ** 32
    frames = torch.zeros(N, 224, 224, 3, dtype=torch.uint8, device=dev)
    rows = [0, 14267, 28533, 28539]
    g = torch.Generator().manual_seed(7)
    written = torch.randint(1, 256, (4, 224, 224, 3), dtype=torch.uint8, generator=g)          # no zero byte: never a blank frame
    for r, f in zip(rows, written):
        frames[r].copy_(f)
    store = _store(frames)
    index = torch.tensor(rows, dtype=torch.int64)
    aug = DeviceFrameAugment()
    for params in (FrameParams.identity(4, 224, 224), _random_params(4, 224, 224, seed=3)):
        (out, out8), (want, want8) = _both(store, index, aug, params)
        assert torch.equal(out8, want8) and torch.equal(out, want)
    ident8 = store.transform(index, aug, FrameParams.identity(4, 224, 224), return_uint8=True)[1]
    assert torch.equal(ident8.cpu(), written)             # and they are the frames that were written, not rows of zeros
    del store, frames
    torch.cuda.empty_cache()


def test_bad_index_is_a_host_error(dev):
    from multimodal.augment import DeviceFrameAugment
    store = _store(torch.zeros(7, 32, 32, 3, dtype=torch.uint8, device=dev))
    aug = DeviceFrameAugment()
    for bad in ([7], [-1], [0, 7, 2]):
        for where in ("cpu", dev):
            with pytest.raises(IndexError, match="outside the store's 0..6"):
                store.transform(torch.tensor(bad, dtype=torch.int64, device=where), aug)
    assert store.transform(torch.tensor([6, 0], dtype=torch.int64), aug).shape == (2, 3, 224, 224)


# ---- the data module and the entry points on a dataset on disk ---------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = SC.materialize(tmp_path_factory.mktemp("saycam"), SC.load_committed_metadata(GOLDEN))
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.append(tools)
    store = os.path.join(root, "frames.npy")
    importlib.import_module("pack_frames").pack(root, store, ["eval_dev.json", "eval_test.json"], workers=1)
    return root, store


def _module(argv):
    import train
    from multimodal.multimodal_saycam_data_module import MultiModalSAYCamDataModule
    with contextlib.redirect_stdout(io.StringIO()):
        dm = MultiModalSAYCamDataModule(train._setup_parser().parse_args(argv))
        dm.setup()
    return dm


def _to(batch, dev):
    return tuple(b.to(dev) if torch.is_tensor(b) else b for b in batch)


def test_store_path_equals_device_frames_path(dev, dataset):
    from multimodal.augment import DeviceFrameAugment
    root, store_path = dataset
    G = load_golden("saycam_data")
    names = [str(n) for n in G["train_frame_names"]]
    base = f"--dataset saycam --data_dir {root} --eval_metadata_filename eval_dev.json {SMALL}".split()
    for extra in ([], ["--augment_frames"], ["--multiple_frames"]):
        by_store = _module(base + extra + ["--frame_store", store_path])
        by_u8 = _module(base + extra + ["--device_frames"])
        assert by_store.frame_store.frames.is_cuda and len(by_store.frame_store) == 28
        batches = []
        for dm in (by_store, by_u8):
            torch.manual_seed(11)                          # the loader's shuffle
            random.seed(0)                                 # --multiple_frames' choice of frame
            batches.append(next(iter(dm.train_dataloader(batch_size=6))))
        (idx, tok, ln, raw), (u8, tok2, ln2, raw2) = batches
        assert idx.dtype == torch.int64 and idx.shape == (6,) and u8.shape == (6, 224, 224, 3)
        assert torch.equal(tok, tok2) and torch.equal(ln, ln2) and raw == raw2
        out = []
        for dm, b in ((by_store, batches[0]), (by_u8, batches[1])):
            torch.manual_seed(5)                           # the augmentation's draws
            random.seed(5)
            out.append(dm.on_after_batch_transfer(_to(b, dev), 0, training=True)[0])
        assert out[0].shape == (6, 3, 224, 224) and torch.equal(out[0], out[1])
        if "--augment_frames" in extra:                    # given the same FrameParams explicitly, too; and val keeps the base transform
            aug = DeviceFrameAugment()
            p = aug.sample_params_sequential(6, 224, 224)
            assert torch.equal(by_store.frame_store.transform(idx, aug, p), aug(u8.to(dev), p))
            assert not torch.equal(out[0], by_u8.on_after_batch_transfer(_to(batches[1], dev), 0, training=False)[0])
        if "--multiple_frames" in extra:                   # both paths pick the frames the reference picks after random.seed(0)
            for dm in (by_store, by_u8):
                random.seed(0)
                b = next(iter(dm.train_dataloader(shuffle=False, batch_size=6)))
                want = [names[f] for f in G["train_multiple_frames_seed_0"].tolist()]
                if dm is by_store:
                    assert b[0].tolist() == [dm.frame_store.index_of(f"train_5fps/{n}") for n in want]
                else:
                    from PIL import Image
                    for got, n in zip(b[0], want):
                        assert np.array_equal(got.numpy(), np.array(Image.open(os.path.join(root, "train_5fps", n)).convert("RGB")))
        # the pair loader of val and the trial loader
        for di in (0, 1):
            a, b = (next(iter(dm.val_dataloader()[di])) for dm in (by_store, by_u8))
            outs = []
            for dm, x in ((by_store, a), (by_u8, b)):
                torch.manual_seed(5)
                random.seed(5)
                outs.append(dm.on_after_batch_transfer(_to(x, dev), di, training=False)[0])
            assert outs[0].shape == ((1, 4, 3, 224, 224) if di else (3, 3, 224, 224)) and torch.equal(outs[0], outs[1])
            assert torch.equal(a[1], b[1])
            if di and not extra:                           # the host path gives the same trial
                host = next(iter(_module(base).val_dataloader()[1]))[0]
                assert torch.equal(outs[0].cpu(), host)


def test_train_entry_on_a_saycam_directory(dev, dataset, tmp_path, monkeypatch):
    import train
    root, store_path = dataset
    monkeypatch.chdir(tmp_path)
    argv = f"--dataset saycam --data_dir {root} --frame_store {store_path} --eval_metadata_filename eval_dev.json {SMALL} " \
           "--fast_dev_run --checkpoint_callback False --multiple_frames --augment_frames".split()
    with contextlib.redirect_stdout(io.StringIO()):
        trainer, lit = train.main(argv)
    m = trainer.logged_metrics
    assert trainer.global_step == 1
    for k in ("train_loss", "val_loss", "val_accuracy"):
        assert k in m and np.isfinite(float(m[k])), (k, sorted(m))


@pytest.fixture(scope="module")
def checkpoint(dataset, tmp_path_factory):
    """a (nearly) random-init checkpoint written by train.py on the dataset, host frame path"""
    import train
    root, _ = dataset
    work = tmp_path_factory.mktemp("work")
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    cwd = os.getcwd()
    os.chdir(work)
    try:
        argv = f"--dataset saycam --data_dir {root} --eval_metadata_filename eval_dev.json {SMALL} --max_epochs 1 " \
               f"--limit_train_batches 1 --limit_val_batches 1 --checkpoint_callback True --exp_name {exp}".split()
        with contextlib.redirect_stdout(io.StringIO()):
            train.main(argv)
    finally:
        os.chdir(cwd)
    return str(work), exp


@pytest.mark.parametrize("eval_type", ["image", "text"])
def test_eval_entry_on_a_saycam_directory(dev, dataset, checkpoint, monkeypatch, eval_type):
    import eval as ev
    root, store_path = dataset
    work, exp = checkpoint
    monkeypatch.chdir(work)
    base = ["--checkpoint", exp, "--eval_dataset", "saycam", "--data_dir", root, "--eval_metadata_filename", "eval_test.json",
            "--stage", "test", "--eval_type", eval_type, "--trial_batch", "3", "--save_predictions"]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = ev.main(ev._parser().parse_args(base))
        stored = ev.main(ev._parser().parse_args(base + ["--frame_store", store_path]))
    trials = SC.metadata()["eval_test.json"]["data"]
    assert len(stored) == len(trials) == 4
    for r, p, t in zip(stored, plain, trials):
        assert r["categories"] == [t["target_category"]] + t["foil_categories"] and r["eval_dataset"] == "saycam"
        assert len(r["logits"]) == 4 and np.isfinite(r["logits"]).all() and abs(sum(r["logits"]) - 1.0) < 1e-5
        assert r["logits"] == p["logits"] and r["pred"] == p["pred"]            # the same frames, bit for bit, give the same logits
    name = f"results/saycam/embedding_frozen_random_init_seed_0_{eval_type}_saycam_test_eval_predictions.json"
    with open(os.path.join(work, name)) as f:
        assert json.load(f)["data"] == stored
