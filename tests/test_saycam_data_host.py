"""CPU: the SAYCam-layout data module against the reference's own datasets (tests/golden/saycam_data.npz, written by
tools/gen_golden_saycam_data.py), its loaders, path resolution, the host transform, and tools/pack_frames.py + FrameStore."""
import argparse
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
from PIL import Image

import saycam_common as SC
from conftest import GOLDEN, ROOT, load_golden

from multimodal.multimodal_data_module import (IMAGENET_MEAN, IMAGENET_STD, FrameSource, HostFrameTransform, LabeledSEvalDataset,
                                               LabeledSTextEvalDataset, load_data, multiModalDataset_collate_fn, read_vocab)
from multimodal.multimodal_saycam_data_module import MultiModalSAYCamDataModule, MultiModalSAYCamDataset


def _tool(name):
    """a module of tools/, importable by name (pack_frames' decoding processes import it again)"""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.append(tools)
    return importlib.import_module(name)


@pytest.fixture(scope="module")
def G():
    return load_golden("saycam_data")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return SC.materialize(tmp_path_factory.mktemp("saycam"), SC.load_committed_metadata(GOLDEN))


def _module(data_dir, **kw):
    base = dict(data_dir=data_dir, batch_size=4, val_batch_size=2, num_workers=0, eval_metadata_filename="eval_dev.json")
    base.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        dm = MultiModalSAYCamDataModule(argparse.Namespace(**base))
        dm.prepare_data()
        dm.setup()
    return dm


def _decode(path):
    return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)


def _normalised(u8):
    x = torch.from_numpy(u8).permute(2, 0, 1).float() / 255.0
    return (x - torch.tensor(IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(IMAGENET_STD).view(3, 1, 1)


def test_committed_metadata_is_the_generators():
    assert SC.load_committed_metadata(GOLDEN) == SC.metadata()
    lens = [len(d["utterance"].split()) + 2 for d in SC.metadata()["train.json"]["data"]]
    assert max(lens) > 25 and any(len(d["frame_filenames"]) > 1 for d in SC.metadata()["train.json"]["data"])


def test_pair_datasets_and_collate_match_the_reference(G, data_dir):
    vocab = read_vocab()
    names = [str(n) for n in G["train_frame_names"]]
    for split in ("train", "train_shuffled", "val", "test"):
        data = load_data(os.path.join(data_dir, split + ".json"))
        ds = MultiModalSAYCamDataset(data, vocab, False, HostFrameTransform(False), frames=FrameSource(data_dir))
        items = [ds[i] for i in range(len(ds))]
        assert [it[2] for it in items] == G[f"{split}_lengths"].tolist()
        assert torch.equal(torch.cat([it[1] for it in items]), G[f"{split}_ids"]) and items[0][1].dtype == torch.int64
        assert [it[3] for it in items] == [[d["utterance"]] for d in data]
        for it, f in zip(items, G[f"{split}_frame"].tolist()):
            assert torch.equal(it[0], _normalised(_decode(os.path.join(data_dir, "train_5fps", names[f]))))
        img, idxs, length, raw = multiModalDataset_collate_fn(items)
        assert torch.equal(idxs, G[f"{split}_batch_ids"]) and torch.equal(length, G[f"{split}_batch_lengths"])
        assert img.shape == (len(ds), 3, 224, 224) and img.dtype == torch.float32 and raw == [it[3] for it in items]
    assert int(G["train_lengths"].max()) > 25 and int(G["train_batch_lengths"].max()) == 25        # the truncation is exercised
    assert 1 in G["train_ids"].tolist()                                                             # and so is <unk>


def test_multiple_frames_draws_the_references_frames(G, data_dir):
    vocab = read_vocab()
    names = [str(n) for n in G["train_frame_names"]]
    data = load_data(os.path.join(data_dir, "train.json"))
    for mode in ("uint8", "host"):
        ds = MultiModalSAYCamDataset(data, vocab, True, HostFrameTransform(False), frames=FrameSource(data_dir, mode))
        for seed in (0, 1):
            random.seed(seed)
            got = [ds[i][0] for i in range(len(ds))]
            for img, f in zip(got, G[f"train_multiple_frames_seed_{seed}"].tolist()):
                u8 = _decode(os.path.join(data_dir, "train_5fps", names[f]))
                assert torch.equal(img, torch.from_numpy(u8) if mode == "uint8" else _normalised(u8))
    assert G["train_multiple_frames_seed_0"].tolist() != G["train_multiple_frames_seed_1"].tolist()


@pytest.mark.parametrize("stage", ["dev", "test"])
@pytest.mark.parametrize("sos_eos", [False, True])
def test_eval_datasets_match_the_reference(G, data_dir, stage, sos_eos):
    vocab = read_vocab()
    trials = load_data(os.path.join(data_dir, f"eval_{stage}.json"))
    tag = f"eval_{stage}_sos_eos_{int(sos_eos)}"
    src = FrameSource(data_dir)
    ds = LabeledSEvalDataset(trials, vocab, HostFrameTransform(False), sos_eos, frames=src)
    items = [ds[i] for i in range(len(ds))]
    assert torch.equal(torch.stack([it[1] for it in items]), G[f"{tag}_image_labels"]) and items[0][1].dtype == torch.int64
    assert [it[2] for it in items] == G[f"{tag}_image_lengths"].tolist()
    for it, t in zip(items, trials):                      # the target image first, then the foils in their order
        want = [t["target_img_filename"]] + t["foil_img_filenames"]
        assert it[0].shape == (4, 3, 224, 224) and it[3] == [t["target_category"]]
        assert torch.equal(it[0], torch.stack([_normalised(_decode(os.path.join(data_dir, w))) for w in want]))
    b = multiModalDataset_collate_fn(items[:1])
    assert torch.equal(b[1], G[f"{tag}_image_batch_labels"]) and torch.equal(b[2], G[f"{tag}_image_batch_lengths"])
    assert b[0].shape == (1, 4, 3, 224, 224)
    ds = LabeledSTextEvalDataset(trials, vocab, HostFrameTransform(False), sos_eos, frames=src)
    items = [ds[i] for i in range(len(ds))]
    assert torch.equal(torch.stack([it[1] for it in items]), G[f"{tag}_text_labels"])
    assert [it[2] for it in items] == G[f"{tag}_text_lengths"].tolist()
    for it, t in zip(items, trials):
        assert it[0].shape == (1, 3, 224, 224) and it[3] == [t["target_category"]]
        assert torch.equal(it[0][0], _normalised(_decode(os.path.join(data_dir, t["target_img_filename"]))))
    b = multiModalDataset_collate_fn(items[:1])
    assert torch.equal(b[1], G[f"{tag}_text_batch_labels"]) and torch.equal(b[2], G[f"{tag}_text_batch_lengths"])


def test_loaders_of_the_module(G, data_dir):
    dm = _module(data_dir)
    val = dm.val_dataloader()
    assert len(val) == 2 and val[0].batch_size == 2 and val[1].batch_size == 1
    assert isinstance(val[1].dataset, LabeledSEvalDataset) and len(dm.test_dataloader()) == 2
    img, idxs, length, raw = next(iter(val[0]))
    assert img.shape == (2, 3, 224, 224) and torch.equal(length, G["val_batch_lengths"][:2])
    trial = next(iter(val[1]))
    assert trial[0].shape == (1, 4, 3, 224, 224) and trial[3] == [["ball"]]
    tr = dm.train_dataloader(shuffle=False)
    assert tr.batch_size == 4 and torch.equal(next(iter(tr))[1], G["train_batch_ids"][:4])
    assert dm.train_dataloader().sampler.__class__.__name__ == "RandomSampler"
    four = _module(data_dir, test_while_val=True).val_dataloader()
    assert len(four) == 4 and [l.batch_size for l in four] == [2, 1, 2, 1]
    assert four[2].dataset is not four[0].dataset and four[3].dataset.data[0]["target_img_filename"].startswith("eval/test/")
    # the trial datasets carry the TRAINING transform, the val / test pairs the base one (reference :339-360, :181-211)
    aug = _module(data_dir, augment_frames=True)
    assert aug.eval_datasets["val"].transform is aug.transform and aug.transform.augment_frames
    assert aug.datasets["val"].transform is aug.base_transform and not aug.base_transform.augment_frames
    assert aug.datasets["train"].transform is aug.transform
    text = _module(data_dir, eval_type="text")
    assert isinstance(text.val_dataloader()[1].dataset, LabeledSTextEvalDataset)


def test_shuffle_utterances_reads_train_shuffled(G, data_dir):
    dm = _module(data_dir, shuffle_utterances=True)
    assert [d["utterance"] for d in dm.datasets["train"].data] == [d["utterance"] for d in SC.metadata()["train_shuffled.json"]["data"]]
    assert torch.equal(next(iter(dm.train_dataloader(shuffle=False, batch_size=6)))[1], G["train_shuffled_batch_ids"])
    assert [d["utterance"] for d in dm.datasets["val"].data] == [d["utterance"] for d in SC.metadata()["val.json"]["data"]]


def test_data_dir_from_the_environment_and_own_vocab(data_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("CVCL_DATA_DIR", data_dir)
    dm = _module(None)
    assert dm.data_dir == data_dir and len(dm.read_vocab()) == 2350
    monkeypatch.delenv("CVCL_DATA_DIR")
    with pytest.raises(ValueError, match="data_dir"):
        MultiModalSAYCamDataModule(argparse.Namespace(data_dir=None))
    own = SC.materialize(tmp_path / "own", SC.metadata())
    with open(os.path.join(own, "vocab.json"), "w") as f:
        json.dump({"<pad>": 0, "<unk>": 1, "<sos>": 2, "<eos>": 3, "ball": 4, "car": 5, "cat": 6, "dog": 7}, f)
    dm = _module(own)
    assert len(dm.read_vocab()) == 8 and dm.datasets["train"][0][1].tolist() == [2, 1, 1, 1, 4, 3]


def test_relative_and_absolute_eval_paths(data_dir, tmp_path):
    meta = SC.metadata()
    elsewhere = tmp_path / "elsewhere" / "abs_target.png"
    trials = meta["eval_dev.json"]["data"]
    trials[0]["target_img_filename"] = str(elsewhere)               # absolute: used as written; the foils stay relative
    root = SC.materialize(tmp_path / "d", meta)
    Image.fromarray(SC.frame_pixels("abs_target")).save(elsewhere)  # (after materialize, which writes every named frame)
    dm = _module(root)
    imgs = dm.eval_datasets["val"][0][0]
    assert torch.equal(imgs[0], _normalised(SC.frame_pixels("abs_target")))
    assert torch.equal(imgs[1], _normalised(SC.frame_pixels(trials[0]["foil_img_filenames"][0])))
    assert dm.eval_datasets["test"].data[0]["target_img_filename"] == "eval/test/ball/img_0.png"       # dev -> test file


def test_host_augment_uses_the_sequential_draws(data_dir):
    """--augment_frames on the host: the draws of DeviceFrameAugment.sample_params_sequential, the pixels through Pillow"""
    from PIL import ImageFilter
    from multimodal.augment import DeviceFrameAugment
    path = os.path.join(data_dir, "train_5fps", "clip0_00.jpg")
    for seed in (0, 3):
        torch.manual_seed(seed)
        random.seed(seed)
        got = HostFrameTransform(True)(Image.open(path).convert("RGB"))
        torch.manual_seed(seed)
        random.seed(seed)
        p = DeviceFrameAugment(True).sample_params_sequential(1, 224, 224)
        top, left, h, w = (int(v) for v in p.crop[0])
        im = Image.open(path).convert("RGB").crop((left, top, left + w, top + h)).resize((224, 224), Image.BILINEAR)
        if float(p.sigma[0]) > 0:
            im = im.filter(ImageFilter.GaussianBlur(radius=float(p.sigma[0])))
        if int(p.flip[0]):
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert torch.equal(got, _normalised(np.array(im)))


def test_device_frames_mode_yields_uint8(data_dir):
    dm = _module(data_dir, device_frames=True)
    img = next(iter(dm.train_dataloader(shuffle=False)))[0]
    assert img.dtype == torch.uint8 and img.shape == (4, 224, 224, 3)
    assert torch.equal(img[0], torch.from_numpy(_decode(os.path.join(data_dir, "train_5fps", "clip0_00.jpg"))))
    assert next(iter(dm.val_dataloader()[1]))[0].shape == (1, 4, 224, 224, 3)


# ---- tools/pack_frames.py + FrameStore ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed(data_dir, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("store") / "frames.npy")
    n, shape = _tool("pack_frames").pack(data_dir, out, ["eval_dev.json", "eval_test.json"], workers=2)
    return out, n, shape


def test_pack_frames_holds_pillows_decode(data_dir, packed):
    from multimodal.frame_store import FrameStore
    out, n, shape = packed
    train, ev = SC.frame_names(SC.metadata())
    assert n == len(train) + len(ev) and shape == (224, 224, 3)
    arr, index = FrameStore.open_memmap(out)
    assert arr.shape == (n, 224, 224, 3) and arr.dtype == np.uint8 and sorted(index.values()) == list(range(n))
    store = FrameStore.load(out, "cpu")
    assert len(store) == n and (store.height, store.width) == (224, 224) and store.frames.dtype == torch.uint8
    for key, path in (("train_5fps/clip1_02.jpg", os.path.join(data_dir, "train_5fps", "clip1_02.jpg")),      # one JPEG
                      ("eval/dev/cat/img_0.png", os.path.join(data_dir, "eval/dev/cat/img_0.png"))):           # and one PNG
        want = _decode(path)
        assert np.array_equal(arr[index[key]], want) and np.array_equal(store.frames[store.index_of(key)].numpy(), want)
    for key in index:                                     # and every other frame
        assert np.array_equal(arr[index[key]], _decode(os.path.join(data_dir, key)))
    with pytest.raises(KeyError, match="train_5fps/nope.jpg"):
        store.index_of("train_5fps/nope.jpg")
    with open(out + ".json") as f:
        side = json.load(f)
    assert side["H"] == 224 and side["W"] == 224 and side["index"] == index


def test_store_index_checks_and_no_cpu_pixel_path(packed):
    from multimodal import _hip
    from multimodal.augment import DeviceFrameAugment
    from multimodal.frame_store import FrameStore
    store = FrameStore.load(packed[0], "cpu")
    for bad in ([len(store)], [-1], [0, 3, len(store) + 5]):
        with pytest.raises(IndexError, match="outside the store"):
            store.transform(torch.tensor(bad, dtype=torch.int64), DeviceFrameAugment(False))
    with pytest.raises(_hip.CvclError, match="int64"):
        store.transform(torch.tensor([0], dtype=torch.int32), DeviceFrameAugment(False))
    with pytest.raises(_hip.CvclError, match="no CPU pixel path"):
        store.transform(torch.tensor([0], dtype=torch.int64), DeviceFrameAugment(False))


def test_module_over_a_store_yields_indices_and_resolves_at_setup(data_dir, packed, tmp_path):
    from multimodal.frame_store import FrameStore
    dm = _module(data_dir, frame_store=packed[0], num_workers=3)
    store = dm.frame_store
    assert isinstance(store, FrameStore) and len(store) == packed[1]
    tr = dm.train_dataloader(shuffle=False)
    assert tr.num_workers == 0
    img = next(iter(tr))[0]
    assert img.dtype == torch.int64 and img.shape == (4,)
    assert img.tolist() == [store.index_of(f"train_5fps/{d['frame_filenames'][0]}") for d in dm.datasets["train"].data[:4]]
    trial = next(iter(dm.val_dataloader()[1]))
    t0 = dm.eval_datasets["val"].data[0]
    assert trial[0].dtype == torch.int64 and trial[0].shape == (1, 4)
    assert trial[0][0].tolist() == [store.index_of(k) for k in [t0["target_img_filename"]] + t0["foil_img_filenames"]]
    text = _module(data_dir, frame_store=packed[0], eval_type="text")
    assert next(iter(text.val_dataloader()[1]))[0].shape == (1, 1)
    # a store without the evaluation frames: refused at setup, by name, before any batch
    small = str(tmp_path / "pairs_only.npy")
    _tool("pack_frames").pack(data_dir, small, [], workers=1)
    with pytest.raises(KeyError, match="eval/dev/ball/img_0.png"):
        _module(data_dir, frame_store=small)


def test_wrong_size_frame_is_refused_by_name(tmp_path):
    meta = SC.metadata()
    root = SC.materialize(tmp_path / "d", meta)
    bad = os.path.join(root, "train_5fps", "clip1_01.jpg")
    Image.fromarray(SC.frame_pixels("x", 200, 224)).save(bad)
    out = str(tmp_path / "s.npy")
    with pytest.raises(SystemExit, match=r"clip1_01\.jpg.*200 x 224"):
        _tool("pack_frames").pack(root, out, [], workers=2)
    assert not os.path.exists(out) and not os.path.exists(out + ".json")


def test_entry_points_still_exit_without_a_data_directory(monkeypatch):
    import eval as ev
    import train
    monkeypatch.delenv("CVCL_DATA_DIR", raising=False)
    for argv in (["--dataset", "saycam"], ["--dataset", "coco"], ["--dataset", "coco", "--data_dir", "/somewhere"]):
        with pytest.raises(SystemExit, match="synthetic"):
            train.main(argv)
    for argv in (["--checkpoint", "c.ckpt", "--eval_dataset", "saycam"], ["--checkpoint", "c.ckpt", "--eval_dataset", "object_categories"],
                 ["--checkpoint", "c.ckpt", "--eval_dataset", "object_categories", "--data_dir", "/somewhere"],
                 ["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "b.txt", "--eval_dataset", "saycam", "--data_dir", "/somewhere"]):
        with pytest.raises(SystemExit, match="--eval_dataset synthetic"):
            ev.main(ev._parser().parse_args(argv))
    a = train._setup_parser().parse_args(["--dataset", "saycam", "--data_dir", "D", "--frame_store", "S", "--multiple_frames"])
    assert a.data_dir == "D" and a.frame_store == "S" and a.multiple_frames
    e = ev._parser().parse_args(["--eval_dataset", "saycam", "--data_dir", "D", "--frame_store", "S"])
    assert e.data_dir == "D" and e.frame_store == "S"
