"""GPU: the map-faithfulness kernels (csrc/faithfulness.hip) and multimodal/map_faithfulness.py against the numpy / float64
restatement of tests/faithfulness_common.py, whose docstring derives the bounds: ranks and perturbed frames exactly, the blur, the
paired dot and the areas within their fp32 bounds, deletion_insertion end to end against frames built with numpy and encoded by the
model's own encode_image in the same chunk partition, the script and the bench tool in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import faithfulness_common as FC
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = -777.25
_MAPS = {}


def _F():
    from multimodal import map_faithfulness as F
    return F


def _maps(content, M, H, W):
    """a case's maps and reference ranks, computed once (the largest M; smaller M are its leading maps)"""
    key = (content, H, W)
    if key not in _MAPS:
        m = FC.make_maps(content, 70, H, W)
        _MAPS[key] = (m, FC.ranks(m))
    m, r = _MAPS[key]
    return m[:M], r[:M]


# ---- ranks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", FC.CONTENTS)
@pytest.mark.parametrize("H,W", [(1, 1), (7, 7), (5, 13), (31, 33), (32, 32), (33, 32), (224, 224), (256, 256)])
def test_ranks_equal_the_stable_descending_argsort(content, H, W):
    for M in (1, 3, 70):
        m, want = _maps(content, M, H, W)
        got = _F().pixel_ranks(torch.from_numpy(m).to(DEV))
        assert got.dtype == torch.int32 and tuple(got.shape) == (M, H, W)
        got = got.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"M {M}: {len(bad)} ranks differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def test_ranks_of_a_flat_view_and_twice_the_same_bits():
    m, want = _maps("gauss", 3, 31, 33)
    d = torch.from_numpy(m).to(DEV).view(3, -1)
    a, b = _F().pixel_ranks(d), _F().pixel_ranks(d)
    assert tuple(a.shape) == (3, 31 * 33) and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want.reshape(3, -1))


# ---- perturb ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 9), (224, 224)])
@pytest.mark.parametrize("with_baseline", [False, True])
def test_perturb_is_the_select_bit_for_bit(H, W, with_baseline):
    F = _F()
    rng = np.random.default_rng([H, W])
    N, M, C, HW = 2, 3, 3, H * W
    images = rng.standard_normal((N, C, H, W)).astype(np.float32)
    base = rng.standard_normal((N, C, H, W)).astype(np.float32) if with_baseline else None
    rk = FC.ranks(FC.make_maps("relu", M, H, W, seed=3))
    iom = [1, 0, 1]
    counts = [0, 1, HW // 3, HW - 1, HW]
    item_map = np.array([m for mode in (0, 1) for k in counts for m in range(M)], dtype=np.int32)
    item_count = np.array([k for mode in (0, 1) for k in counts for m in range(M)], dtype=np.int32)
    item_mode = np.array([mode for mode in (0, 1) for k in counts for m in range(M)], dtype=np.int32)
    n = len(item_map)
    want = FC.perturb(images, base, rk, iom, item_map, item_count, item_mode)
    buf = torch.full((n + 1, C, H, W), CANARY, dtype=torch.float32, device=DEV)
    d_base = None if base is None else torch.from_numpy(base).to(DEV)
    out = F.perturb(torch.from_numpy(images).to(DEV), d_base, torch.from_numpy(rk).to(DEV), iom, item_map, item_count, item_mode, out=buf[:n])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, C, H, W)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((buf[n] == CANARY).all()), "the canary behind the output was written"
    # an output that is not 16-byte aligned takes the scalar path and gives the same bits
    shifted = torch.full((n * C * HW + 1 + 4,), CANARY, dtype=torch.float32, device=DEV)
    view = shifted[1:1 + n * C * HW].view(n, C, H, W)
    F.perturb(torch.from_numpy(images).to(DEV), d_base, torch.from_numpy(rk).to(DEV), iom, item_map, item_count, item_mode, out=view)
    assert np.array_equal(view.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert float(shifted[0]) == CANARY and bool((shifted[1 + n * C * HW:] == CANARY).all())


def test_perturb_refuses_out_of_range_items_on_the_host():
    F = _F()
    from multimodal import _hip as H
    img = torch.zeros(2, 3, 7, 9, device=DEV)
    rk = torch.zeros(3, 7, 9, dtype=torch.int32, device=DEV)
    out = torch.full((1, 3, 7, 9), CANARY, device=DEV)
    for iom, im, ic, mode, msg in (([1, 0, 1], [3], [0], [0], "item_map"), ([1, 0, 1], [0], [64], [0], "item_count"),
                                   ([1, 0, 2], [0], [0], [0], "image_of_map"), ([1, 0, 1], [0], [0], [2], "item_mode")):
        with pytest.raises(H.CvclError, match=msg):
            F.perturb(img, None, rk, iom, im, ic, mode, out=out)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())


# ---- blur, pair dot, auc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,k,sigma", [(7, 9, 5, 1.5), (224, 224, 11, 5.0)])
def test_blur_against_float64(H, W, k, sigma):
    x = np.random.default_rng([H, k]).standard_normal((2, 3, H, W)).astype(np.float32)
    got = _F().gaussian_blur(torch.from_numpy(x).to(DEV), k, sigma).cpu().numpy().astype(np.float64)
    err, bound = float(np.abs(got - FC.blur(x, k, sigma)).max()), FC.blur_bound(k, x)
    print(f"blur {H}x{W} k {k}: max error {err:.3e}, bound {bound:.3e}")
    assert got.shape == x.shape and err <= bound


@pytest.mark.parametrize("E", [1, 33, 512])
def test_pair_dot_against_float64(E):
    rng = np.random.default_rng(E)
    R, M = 37, 5
    rows, targets = rng.standard_normal((R, E)).astype(np.float32), rng.standard_normal((M, E)).astype(np.float32)
    t = rng.integers(0, M, R).astype(np.int32)
    got = _F().pair_dot(torch.from_numpy(rows).to(DEV), torch.from_numpy(targets).to(DEV), torch.from_numpy(t).to(DEV)).cpu().numpy()
    err, bound = np.abs(got.astype(np.float64) - FC.pair_dot(rows, targets, t)), FC.pair_dot_bound(rows, targets, t)
    print(f"pair dot E {E}: max error / bound {float((err / bound).max()):.3f}")
    assert got.dtype == np.float32 and (err <= bound).all()


@pytest.mark.parametrize("K,S,M,HW", [(2, 4, 3, 49), (2, 14, 70, 50176), (1, 1, 1, 7)])
def test_auc_against_float64(K, S, M, HW):
    y = np.random.default_rng([K, S, M]).standard_normal((K, S + 1, M)).astype(np.float32)
    x = (np.asarray(FC.step_counts(HW, S), dtype=np.float64) / HW).astype(np.float32)
    got = _F().curve_auc(torch.from_numpy(y).to(DEV), torch.from_numpy(x).to(DEV)).cpu().numpy()
    err, bound = float(np.abs(got.astype(np.float64) - FC.auc(y, x)).max()), FC.auc_bound(y)
    print(f"auc S {S}: max error {err:.3e}, bound {bound:.3e}")
    assert got.shape == (K, M) and err <= bound
    const = _F().curve_auc(torch.full((K, S + 1, M), 0.625, device=DEV), torch.from_numpy(x).to(DEV))
    assert float((const - 0.625).abs().max()) <= (S + 4) * FC.EPS * 0.625


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
SIZE, STEPS = 64, 4


@pytest.fixture(scope="module")
def lit():
    import argparse
    from multimodal.alignment import build_model
    return build_model(argparse.Namespace(checkpoint=None, random_init=True, precision="32", seed=0), DEV)


@pytest.fixture(scope="module")
def pairs(lit):
    """4 frames with one single-word utterance each -> (images, texts, lengths, targets)"""
    from multimodal.alignment import SYNTHETIC_WORDS, word_ids
    from multimodal.multimodal_data_module import read_vocab
    g = torch.Generator(device=DEV).manual_seed(11)
    images = torch.randn(4, 3, SIZE, SIZE, device=DEV, generator=g)
    texts = torch.tensor(word_ids(SYNTHETIC_WORDS[:4], read_vocab()), dtype=torch.long, device=DEV).view(4, 1)
    lengths = torch.ones(4, dtype=torch.long, device=DEV)
    with torch.no_grad():
        targets = lit.model.encode_text(texts, lengths)[0].float().contiguous()
    return images, texts, lengths, targets


def _scores_of(lit, frames, targets, item_map, chunk):
    """float64 dots of the model's own features of ``frames`` (numpy), encoded in consecutive chunks -> (scores, bounds)"""
    feats = []
    with torch.no_grad():
        for s in range(0, len(frames), chunk):
            feats.append(lit.model.encode_image(torch.from_numpy(frames[s:s + chunk]).to(DEV))[0].float().cpu().numpy())
    feats, t = np.concatenate(feats), targets.cpu().numpy()
    return FC.pair_dot(feats, t, item_map), FC.pair_dot_bound(feats, t, item_map)


def test_maps_of_gradcam_is_the_diagonal_gradcam_pairs(lit, pairs):
    from multimodal.attention_maps import gradCAM_pairs
    images, texts, lengths, targets = pairs
    F = _F()
    got = F.maps_of(lit, images, texts, lengths, "gradcam")
    want = gradCAM_pairs(lit.vision_encoder, images, targets, normalize_features=bool(lit.model.normalize_features), pairs="diagonal",
                         resize=True)
    assert tuple(got.shape) == (4, SIZE, SIZE) and torch.equal(got, want)
    rnd = F.maps_of(lit, images, texts, lengths, "random", seed=5)
    assert tuple(rnd.shape) == (4, SIZE, SIZE) and torch.equal(rnd, F.maps_of(lit, images, None, None, "random", seed=5))
    assert not torch.equal(rnd, F.maps_of(lit, images, None, None, "random", seed=6)) and 0.0 <= float(rnd.min()) and float(rnd.max()) < 1.0
    with pytest.raises(NotImplementedError):                  # the ViT's producers refuse a ResNeXt encoder as they always do
        F.maps_of(lit, images, texts, lengths, "rollout")
    with pytest.raises(ValueError):
        F.maps_of(lit, images, texts, lengths, "clip")


def test_deletion_insertion_against_numpy_frames_in_the_same_chunks(lit, pairs):
    """chunk = 6 with M = 4 maps: chunks straddle steps and, at items 18 .. 23, the two modes"""
    F = _F()
    images, texts, lengths, targets = pairs
    maps = F.maps_of(lit, images, texts, lengths, "gradcam")
    res = F.deletion_insertion(lit, images, targets, maps, steps=STEPS, chunk=6)
    M, HW = 4, SIZE * SIZE
    assert set(res) == {"deletion", "insertion", "auc_deletion", "auc_insertion", "x"}
    assert tuple(res["deletion"].shape) == tuple(res["insertion"].shape) == (M, STEPS + 1)
    assert tuple(res["auc_deletion"].shape) == tuple(res["auc_insertion"].shape) == (M,) and tuple(res["x"].shape) == (STEPS + 1,)
    counts = FC.step_counts(HW, STEPS)
    assert np.array_equal(res["x"].cpu().numpy(), (np.asarray(counts, dtype=np.float64) / HW).astype(np.float32))
    # the frames, built here from the library's ranks (checked against the restatement) and its blurred baseline (checked above)
    rk = F.pixel_ranks(maps).cpu().numpy()
    assert np.array_equal(rk, FC.ranks(maps.cpu().numpy()))
    img = images.cpu().numpy()
    blurred = F.gaussian_blur(images).cpu().numpy()
    item_map = np.array([m for mode in (0, 1) for k in counts for m in range(M)])
    item_count = np.array([k for mode in (0, 1) for k in counts for m in range(M)])
    item_mode = np.array([mode for mode in (0, 1) for k in counts for m in range(M)])
    frames = np.concatenate([FC.perturb(img, None, rk, None, item_map[:20], item_count[:20], item_mode[:20]),
                             FC.perturb(img, blurred, rk, None, item_map[20:], item_count[20:], item_mode[20:])])
    want, bound = _scores_of(lit, frames, targets, item_map, 6)
    got = torch.stack([res["deletion"].t(), res["insertion"].t()]).cpu().numpy().astype(np.float64)          # [2, S + 1, M]: item order
    err = np.abs(got.reshape(-1) - want)
    print(f"end to end: max error / bound {float((err / bound).max()):.3f}, scores in [{want.min():.4f}, {want.max():.4f}]")
    assert (err <= bound).all()
    auc = torch.stack([res["auc_deletion"], res["auc_insertion"]]).cpu().numpy().astype(np.float64)
    assert float(np.abs(auc - FC.auc(got, res["x"].cpu().numpy())).max()) <= FC.auc_bound(got)
    again = F.deletion_insertion(lit, images, targets, maps, steps=STEPS, chunk=6)
    assert all(torch.equal(res[k], again[k]) for k in res)


def test_curve_ends_with_one_tensor_as_both_baselines(lit, pairs):
    """chunk = M = 4, so every step of either mode is one encoder batch: deletion's last step and insertion's first encode the same
    four baseline frames in the same order, deletion's first and insertion's last the four unperturbed frames.  Small maps (8 x 8,
    resized) under a permuted image_of_map."""
    F = _F()
    images, _, _, targets = pairs
    g = torch.Generator(device=DEV).manual_seed(3)
    maps = torch.rand(4, 8, 8, device=DEV, generator=g)
    base = torch.randn(4, 3, SIZE, SIZE, device=DEV, generator=g)
    iom = [1, 0, 3, 2]
    res = F.deletion_insertion(lit, images, targets, maps, image_of_map=iom, steps=STEPS, deletion_baseline=base, insertion_baseline=base,
                               chunk=4)
    assert torch.equal(res["deletion"][:, -1], res["insertion"][:, 0])
    want, bound = _scores_of(lit, images[iom].cpu().numpy(), targets, np.arange(4), 4)
    for name, got in (("deletion[:, 0]", res["deletion"][:, 0]), ("insertion[:, -1]", res["insertion"][:, -1])):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert (err <= bound).all(), (name, err, bound)
    want, bound = _scores_of(lit, base[iom].cpu().numpy(), targets, np.arange(4), 4)
    assert (np.abs(res["deletion"][:, -1].cpu().numpy().astype(np.float64) - want) <= bound).all()


# ---- the script and the bench tool ---------------------------------------------------------------------------------------------------------
def test_script_writes_both_files(tmp_path):
    out = tmp_path / "faith"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "attention_faithfulness.py"), "--synthetic", "--random_init", "--maps", "gradcam",
                        "random", "--steps", "4", "--out", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out / "faithfulness.json"))
    curves = np.load(out / "curves.npy")
    assert set(rec) == {"kinds", "settings"} and list(rec["kinds"]) == ["gradcam", "random"]
    n = rec["kinds"]["gradcam"]["n"]
    assert n == 8 * 8 and curves.shape == (2, 2, n, 5) and curves.dtype == np.float32 and np.isfinite(curves).all()
    s = rec["settings"]
    assert s["steps"] == 4 and s["chunk"] == 256 and s["precision"] == "32" and s["maps"] == ["gradcam", "random"] and s["synthetic"]
    assert s["deletion_baseline"] == "zero" and s["insertion_baseline"] == "blur" and len(s["classes"]) == 8
    x = np.asarray(FC.step_counts(224 * 224, 4), dtype=np.float64) / (224 * 224)
    for k, kind in enumerate(("gradcam", "random")):
        e = rec["kinds"][kind]
        assert set(e) == {"n", "auc_deletion", "auc_insertion", "auc_difference", "per_class"} and e["n"] == n
        assert set(e["per_class"]) == set(s["classes"]) and all(c["n"] == 8 for c in e["per_class"].values())
        auc = FC.auc(curves[k].transpose(0, 2, 1), x)                                     # [2, n]
        tol = FC.auc_bound(curves[k].transpose(0, 2, 1)) + 1e-12
        assert abs(e["auc_deletion"]["mean"] - auc[0].mean()) <= tol and abs(e["auc_insertion"]["mean"] - auc[1].mean()) <= tol
        assert abs(e["auc_difference"]["mean"] - (auc[1] - auc[0]).mean()) <= 2 * tol
        # both ends encode the unperturbed frame, at another place of the batch: fp32 sums may be ordered differently, no more
        assert np.allclose(curves[k, 0, :, 0], curves[k, 1, :, -1], rtol=0, atol=1e-4 * float(np.abs(curves[k]).max()))
        assert f"{kind}: deletion AUC {e['auc_deletion']['mean']:.4f}" in r.stdout


def test_bench_tool_quick():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_faithfulness.py"), "--quick"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res["ranks_equal_torch"] is True and res["perturb_equal_torch"] is True
    for group, key in (("ranks", "map_ranks_ms"), ("ranks", "torch_sort_scatter_ms"), ("perturb", "perturb_zero_ms"),
                       ("perturb", "torch_where_tensor_ms"), ("blur", "gaussian_blur_ms"), ("call", "deletion_insertion_ms"),
                       ("call", "encoder_only_ms")):
        e = res[group]
        assert 0 < e["min_" + key] <= e[key] <= e["max_" + key], (group, key)
    assert res["call"]["share_outside_encoder"] < 1.0 and res["call"]["perturbed_frames"] == 2 * 3 * 4
