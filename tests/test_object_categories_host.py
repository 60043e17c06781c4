"""CPU: the object-category data module's host side (multimodal/object_categories_data_module.py) on a small dataset on disk -- the
category list, the generated metadata (the reference's keys and order of random draws on a seeded generator), an existing metadata
file, an empty folder, the trial tables of both evaluation types with and without --use_kitty_label -- and eval.py's flags and
exits.  No frame is decoded here: pixels are the device's (tests/test_object_categories_gpu.py)."""
import argparse
import json
import os

import numpy as np
import pytest

import object_categories_common as OC
from conftest import ROOT


def _module(root, **kw):
    from multimodal.object_categories_data_module import ObjectCategoriesDataModule
    return ObjectCategoriesDataModule(argparse.Namespace(data_dir=str(root), eval_type=kw.pop("eval_type", "image"), clip_eval=False, **kw))


def _ready(root, **kw):
    dm = _module(root, **kw)
    dm.prepare_data()
    dm.setup()
    return dm


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return OC.materialize(tmp_path_factory.mktemp("objcat"))


@pytest.fixture(scope="module")
def dm(dataset):
    return _ready(dataset)


def test_public_names_of_the_reference():
    import multimodal.object_categories_data_module as M
    for name in ("ObjectCategoriesEvalDataset", "ObjectCategoriesTextEvalDataset", "ObjectCategoriesDataModule", "_get_object_categories",
                 "_generate_object_category_eval_trial", "_generate_object_category_eval_metadata", "_get_object_category_word_counts"):
        assert hasattr(M, name), name


def test_categories_are_the_vocabulary_folders_sorted(dm, dataset):
    from multimodal.multimodal_data_module import read_vocab
    from multimodal.object_categories_data_module import _get_object_categories
    vocab = read_vocab()
    assert all(c in vocab for c in OC.CATEGORIES + ["kitty"]) and OC.NOT_A_WORD not in vocab
    assert dm.object_categories == OC.CATEGORIES == sorted(OC.CATEGORIES)
    assert _get_object_categories(vocab, os.path.join(dataset, "object_categories")) == OC.CATEGORIES


def _restated_draws(root, seed):
    """the reference's call sequence (object_categories_data_module.py:248-292) on RandomState(seed) over sorted listings"""
    rng = np.random.RandomState(seed)
    folder = os.path.join(os.path.abspath(root), "object_categories")
    files = {c: sorted(os.path.join(folder, c, f) for f in os.listdir(os.path.join(folder, c)) if f.endswith(".jpg")) for c in OC.CATEGORIES}
    out = []
    for target_category in OC.CATEGORIES:
        for target in files[target_category]:
            for i in range(5):
                foil_categories = OC.CATEGORIES.copy()
                foil_categories.remove(target_category)
                foil_categories = rng.choice(foil_categories, size=3, replace=False)
                foil_imgs = [str(rng.choice(files[foil_categories[k]])) for k in range(3)]
                out.append({"trial_num": i, "target_category": target_category, "target_img_filename": target,
                            "foil_categories": [str(c) for c in foil_categories], "foil_img_filenames": foil_imgs})
    return out


def test_generated_metadata(dm, dataset, tmp_path):
    path = os.path.join(dataset, "eval_object_categories.json")
    with open(path) as f:
        data = json.load(f)["data"]
    assert data == dm.data and len(data) == OC.N_TRIALS == 75
    for i, t in enumerate(data):
        assert set(t) == {"trial_num", "target_category", "target_img_filename", "foil_categories", "foil_img_filenames"}
        assert t["trial_num"] == i % 5
        assert t["target_category"] not in t["foil_categories"] and len(set(t["foil_categories"])) == 3 == len(t["foil_img_filenames"])
        assert set(t["foil_categories"]) <= set(OC.CATEGORIES)
        for cat, name in zip([t["target_category"]] + t["foil_categories"], [t["target_img_filename"]] + t["foil_img_filenames"]):
            assert os.path.isfile(name) and os.path.basename(os.path.dirname(name)) == cat
    assert data == _restated_draws(dataset, 0)
    # the same seed on a copy of the dataset gives the same draws; another seed gives others
    again, other = OC.materialize(tmp_path / "again"), OC.materialize(tmp_path / "other")
    strip = lambda root, d: [{k: (v if "filename" not in k else (os.path.relpath(v, root) if isinstance(v, str)
                                                                 else [os.path.relpath(x, root) for x in v])) for k, v in t.items()} for t in d]
    same = strip(again, _ready(again).data)
    assert same == strip(dataset, data)
    different = _ready(other, seed=1).data
    assert strip(other, different) != same and different == _restated_draws(other, 1)


def test_existing_metadata_is_used_unchanged(tmp_path):
    root = OC.materialize(tmp_path / "d")
    trials = [{"trial_num": 0, "target_category": "dog", "target_img_filename": "object_categories/dog/dog_01.jpg",
               "foil_categories": ["cat", "ball", "car"],
               "foil_img_filenames": ["object_categories/cat/cat_00.jpg", os.path.join(root, "object_categories/ball/ball_02.jpg"),
                                      "object_categories/car/car_00.jpg"]}]
    text = json.dumps({"data": trials})
    with open(os.path.join(root, "eval_object_categories.json"), "w") as f:
        f.write(text)
    dm = _ready(root, seed=3)
    assert dm.data == trials and open(os.path.join(root, "eval_object_categories.json")).read() == text
    # relative names resolve against the dataset root, absolute ones stand
    assert dm.frame_files == sorted(os.path.join(root, "object_categories", c, f) for c, f in
                                    (("dog", "dog_01.jpg"), ("cat", "cat_00.jpg"), ("ball", "ball_02.jpg"), ("car", "car_00.jpg")))
    assert all(os.path.isfile(f) for f in dm.frame_files)


def test_empty_category_is_refused_by_name(tmp_path):
    root = OC.materialize(tmp_path / "d", empty="dog")
    with pytest.raises(ValueError, match=r"'dog' has no \.jpg"):
        _module(root).prepare_data()
    assert not os.path.exists(os.path.join(root, "eval_object_categories.json"))


@pytest.mark.parametrize("sos_eos", [False, True])
def test_trial_tables(dataset, sos_eos):
    from multimodal.multimodal_data_module import EOS_TOKEN_ID, SOS_TOKEN_ID, read_vocab
    vocab = read_vocab()
    dm = _ready(dataset, eval_include_sos_eos=sos_eos)
    files = dm.frame_files
    assert files == sorted(set(files)) and len(files) <= 15 and all(os.path.isfile(f) for f in files)
    assert OC.NOT_A_WORD not in "".join(files)
    tabs = {(et, k): dm.trial_table(et, k) for et in ("image", "text") for k in (False, True)}
    for (et, k), tab in tabs.items():
        words = tab["words"]
        assert words == OC.CATEGORIES + (["kitty"] if k else []) and tab["kitty_row"] == (5 if k else None)
        want = [[SOS_TOKEN_ID, vocab[w], EOS_TOKEN_ID] if sos_eos else [vocab[w]] for w in words]
        assert tab["word_rows"].tolist() == want and tab["word_lens"].tolist() == [len(r) for r in want]
        q, c = tab["q_idx"], tab["c_idx"]
        assert q.dtype == c.dtype == np.int32 and q.shape == (75,) and c.shape == (75, 4)
        for i, t in enumerate(dm.data):
            frames = [t["target_img_filename"]] + t["foil_img_filenames"]
            cats = [t["target_category"]] + t["foil_categories"]
            if k and cats[0] == "cat":                     # only the target's own word
                cats[0] = "kitty"
            if et == "image":                              # the word row against frame rows, target first
                assert words[q[i]] == cats[0] and [files[j] for j in c[i]] == frames
            else:                                          # the frame row against word rows, target first
                assert files[q[i]] == frames[0] and [words[j] for j in c[i]] == cats
    for et in ("image", "text"):
        plain, kitty = tabs[et, False], tabs[et, True]
        cat_target = np.array([t["target_category"] == "cat" for t in dm.data])
        assert cat_target.sum() == 15
        if et == "image":
            assert np.array_equal(plain["c_idx"], kitty["c_idx"]) and np.array_equal(plain["q_idx"] != kitty["q_idx"], cat_target)
        else:
            assert np.array_equal(plain["q_idx"], kitty["q_idx"]) and np.array_equal(plain["c_idx"][:, 1:], kitty["c_idx"][:, 1:])
            assert np.array_equal(plain["c_idx"][:, 0] != kitty["c_idx"][:, 0], cat_target)
            assert (plain["c_idx"][:, 1:] == OC.CATEGORIES.index("cat")).any()      # "cat" as a foil stays "cat"
    assert dm.trial_table()["q_idx"].tolist() == tabs["image", False]["q_idx"].tolist()      # the module's own eval_type by default


def test_item_layout_is_declared_for_both_datasets(dataset):
    from multimodal.object_categories_data_module import ObjectCategoriesEvalDataset, ObjectCategoriesTextEvalDataset
    assert isinstance(_ready(dataset, eval_type="image").eval_dataset, ObjectCategoriesEvalDataset)
    text = _ready(dataset, eval_type="text")
    assert isinstance(text.eval_dataset, ObjectCategoriesTextEvalDataset) and len(text.eval_dataset) == 75
    assert text.eval_dataset.eval_include_sos_eos is False and _ready(dataset, eval_include_sos_eos=True).eval_dataset.eval_include_sos_eos


def test_parser_flags_and_exits(monkeypatch, tmp_path):
    import eval as ev
    monkeypatch.delenv("CVCL_DATA_DIR", raising=False)
    a = ev._parser().parse_args(["--eval_dataset", "object_categories", "--object_categories_dir", "O", "--seed", "4", "--no_trial_table"])
    assert a.object_categories_dir == "O" and a.seed == 4 and a.no_trial_table
    d = ev._parser().parse_args([])
    assert d.object_categories_dir is None and d.seed == 0 and d.no_trial_table is False
    assert ev.object_categories_dir(ev._parser().parse_args(["--data_dir", "D"])) == os.path.join("D", "object_categories")
    assert ev.object_categories_dir(a) == "O" and ev.object_categories_dir(d) is None
    for argv in (["--checkpoint", "c.ckpt", "--eval_dataset", "object_categories"],
                 ["--checkpoint", "c.ckpt", "--eval_dataset", "object_categories", "--data_dir", str(tmp_path / "nowhere")],
                 ["--checkpoint", "c.ckpt", "--eval_dataset", "object_categories", "--object_categories_dir", str(tmp_path / "nowhere")],
                 ["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "b.txt", "--eval_dataset", "object_categories"]):
        with pytest.raises(SystemExit, match="use --eval_dataset synthetic.*object_categories/<category>"):
            ev.main(ev._parser().parse_args(argv))
    help_text = ev._parser().format_help()
    for flag in ("--object_categories_dir", "--seed", "--no_trial_table"):
        assert flag in help_text
