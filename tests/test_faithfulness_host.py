"""CPU: the properties of the map-faithfulness yardstick itself (tests/faithfulness_common.py), and the host side of
multimodal/map_faithfulness.py: step_counts, the order of the work items, the script's flags, the layout of faithfulness.json."""
import json

import numpy as np
import pytest

import faithfulness_common as FC


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", FC.CONTENTS)
def test_ranks_are_permutations(content):
    m = FC.make_maps(content, 3, 5, 13)
    r = FC.ranks(m)
    assert r.shape == m.shape and r.dtype == np.int32
    for row in r.reshape(3, -1):
        assert np.array_equal(np.sort(row), np.arange(65))


def test_relu_content_is_mostly_exact_zeros_and_gauss_has_both_zeros_and_subnormals():
    assert (FC.make_maps("relu", 3, 31, 33) == 0).mean() >= 0.6
    g = FC.make_maps("gauss", 3, 31, 33).reshape(-1)
    tiny = np.float32(1.1754944e-38)
    assert (g < 0).any() and ((g == 0) & np.signbit(g)).any() and ((g == 0) & ~np.signbit(g)).any()
    assert ((g != 0) & (np.abs(g) < tiny)).any()
    assert len(np.unique(FC.make_maps("ints", 1, 32, 32))) == 5


def test_ties_go_to_the_lower_flat_index():
    m = np.array([[2.0, 5.0, 2.0, 5.0, -1.0, 2.0]], dtype=np.float32)
    assert FC.ranks(m).tolist() == [[2, 0, 3, 1, 5, 4]]
    assert FC.ranks(np.full((1, 2, 3), 7.0, dtype=np.float32)).reshape(-1).tolist() == [0, 1, 2, 3, 4, 5]


def test_negative_and_positive_zero_tie_and_subnormals_order_by_value():
    m = np.array([[-0.0, 0.0, -0.0, 1e-40, -1e-40, 0.0]], dtype=np.float32)
    assert FC.ranks(m).tolist() == [[1, 2, 3, 0, 5, 4]]


def test_deletion_ends_are_the_image_and_the_baseline():
    rng = np.random.default_rng(0)
    images, base = rng.standard_normal((2, 3, 4, 5)).astype(np.float32), rng.standard_normal((2, 3, 4, 5)).astype(np.float32)
    rk = FC.ranks(rng.standard_normal((3, 4, 5)).astype(np.float32))
    iom = [1, 0, 1]
    out = FC.perturb(images, base, rk, iom, [0, 0, 2, 2], [0, 20, 0, 20], [0, 0, 1, 1])
    assert np.array_equal(out[0], images[1]) and np.array_equal(out[1], base[1])
    assert np.array_equal(out[2], base[1]) and np.array_equal(out[3], images[1])
    one = FC.perturb(images, None, rk, iom, [1], [1], [0])[0]
    top = rk[1] == 0
    assert top.sum() == 1 and (one[:, top] == 0).all() and np.array_equal(one[:, ~top], images[0][:, ~top])


def test_auc_of_a_constant_curve_is_the_constant():
    x = np.asarray(FC.step_counts(49, 4), dtype=np.float64) / 49
    assert np.allclose(FC.auc(np.full((2, 5, 3), 0.625), x), 0.625, rtol=0, atol=1e-15)
    assert np.allclose(FC.auc(np.linspace(0, 1, 5)[None, :, None] * np.ones((1, 5, 2)), np.linspace(0, 1, 5)), 0.5, rtol=0, atol=1e-15)


def test_blur_keeps_a_constant_and_reflects_without_repeating_the_edge():
    assert np.allclose(FC.blur(np.full((2, 7, 9), 3.0), 5, 1.5), 3.0, rtol=0, atol=1e-6)
    # rows (b | a b c d e) with b = 1: column 0 sees b through the taps at -1 (reflected, not the edge a) and at +1
    x = np.tile(np.array([0.0, 1.0, 0.0, 0.0, 0.0]), (3, 1))
    w = FC.gaussian_weights(3, 1.0).astype(np.float64)
    y = FC.blur(x, 3, 1.0)
    assert np.allclose(y[:, 0], w[0] + w[2], rtol=1e-12) and np.allclose(y[:, 4], 0.0) and np.allclose(y[:, 1], w[1], rtol=1e-12)
    assert np.allclose(FC.blur(x.T, 3, 1.0), y.T, rtol=1e-12)


# ---- the library's host side -------------------------------------------------------------------------------------------------------
def test_step_counts_when_hw_is_not_divisible():
    from multimodal import map_faithfulness as F
    assert F.step_counts(49, 4) == [0, 12, 24, 36, 49] == FC.step_counts(49, 4)
    assert F.step_counts(50176, 14) == [s * 3584 for s in range(15)]
    assert F.step_counts(65, 14)[0] == 0 and F.step_counts(65, 14)[-1] == 65 and F.step_counts(65, 14)[1] == 4
    assert F.step_counts(3, 5) == [0, 0, 1, 1, 2, 3]
    with pytest.raises(ValueError):
        F.step_counts(10, 0)


def test_work_items_are_ordered_mode_step_map():
    from multimodal import map_faithfulness as F
    m, k, mode = F.work_items(3, 2, 10)
    assert m.tolist() == [0, 1, 2] * 6 and mode.tolist() == [0] * 9 + [1] * 9
    assert k.tolist() == [0, 0, 0, 5, 5, 5, 10, 10, 10] * 2
    assert m.dtype == k.dtype == mode.dtype == np.int32


def test_parser_flags():
    from multimodal import map_faithfulness as F
    a = F.parser().parse_args(["--synthetic", "--random_init"])
    assert (a.steps, a.chunk, a.precision, a.num_samples_per_class, a.seed) == (14, 256, "32", 8, 0)
    assert a.maps == ["gradcam", "random"] and a.checkpoint is None and a.data_dir is None and not a.use_kitty_label
    a = F.parser().parse_args(["--checkpoint", "m.ckpt", "--data_dir", "d", "--maps", "gradcam", "cls_attention", "rollout", "rollout_discard",
                               "random", "--steps", "4", "--chunk", "6", "--precision", "32-split", "--use_kitty_label", "--out", "o",
                               "--num_samples_per_class", "2", "--seed", "3"])
    assert a.maps == list(F.MAP_KINDS) and (a.steps, a.chunk, a.precision, a.out, a.seed) == (4, 6, "32-split", "o", 3)
    F.check_args(a)
    with pytest.raises(SystemExit):
        F.parser().parse_args(["--maps", "clip"])
    for bad in (["--synthetic"], ["--random_init"], ["--synthetic", "--random_init", "--data_dir", "d"],
                ["--synthetic", "--random_init", "--checkpoint", "c"], ["--synthetic", "--random_init", "--steps", "0"],
                ["--synthetic", "--random_init", "--maps", "random", "random"]):
        with pytest.raises(SystemExit):
            F.check_args(F.parser().parse_args(bad))


def test_json_layout():
    from multimodal import map_faithfulness as F
    d = {"gradcam": [0.1, 0.3, 0.2, 0.6], "random": [0.4, 0.4, 0.4, 0.4]}
    i = {"gradcam": [0.5, 0.7, 0.2, 0.8], "random": [0.4, 0.5, 0.4, 0.5]}
    rec = json.loads(json.dumps(F.faithfulness_record(d, i, [0, 0, 2, 2], ["apple", "ball", "cat"], {"steps": 4})))
    assert set(rec) == {"kinds", "settings"} and rec["settings"] == {"steps": 4} and list(rec["kinds"]) == ["gradcam", "random"]
    g = rec["kinds"]["gradcam"]
    assert set(g) == {"n", "auc_deletion", "auc_insertion", "auc_difference", "per_class"} and g["n"] == 4
    for key in ("auc_deletion", "auc_insertion", "auc_difference"):
        assert set(g[key]) == {"mean", "std"}
    assert np.isclose(g["auc_deletion"]["mean"], 0.3) and np.isclose(g["auc_insertion"]["mean"], 0.55)
    assert np.isclose(g["auc_difference"]["mean"], 0.25) and np.isclose(g["auc_difference"]["std"], np.std([0.4, 0.4, 0.0, 0.2]))
    assert set(g["per_class"]) == {"apple", "cat"}                      # a class without frames is left out
    assert g["per_class"]["cat"] == {"n": 2, "auc_deletion": pytest.approx(0.4), "auc_insertion": pytest.approx(0.5),
                                     "auc_difference": pytest.approx(0.1)}
    assert rec["kinds"]["random"]["auc_deletion"]["std"] == 0.0
    with pytest.raises(ValueError):
        F.faithfulness_record({"k": [0.1]}, {"k": [0.1]}, [0, 1], ["a", "b"], {})
