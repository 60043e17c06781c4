"""GPU: the attention overlays of csrc/overlay.hip (cvcl_attn_overlay, attention_maps.overlay_attention_maps / attention_grid, the
figure script and eval.py --attention_overlays) against getAttMap's arithmetic in float64 on the CPU (tests/overlay_common.py:
F.interpolate bicubic, scipy.ndimage.gaussian_filter, numpy, matplotlib's viridis).  Every device call runs twice on outputs
pre-filled with a canary and must give the same bits.  The bounds and their derivations are in overlay_common's docstring."""
import contextlib
import ctypes
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import overlay_common as OC
from conftest import ROOT

pytestmark = pytest.mark.gpu

EINVAL = -1
CANARY_F, CANARY_U8 = -777.25, 0xAB
_REFS = {}


def _lib():
    from multimodal import _hip as H
    return H, H.lib()


def _ref(name, blur, seed=0):
    """the float64 reference of a case, computed once"""
    key = (name, blur, seed)
    if key not in _REFS:
        N, M, (h, w), (Hh, Ww), idx = OC.CASES[name]
        maps, images = OC.make_maps(M, h, w, seed), OC.make_images(N, Hh, Ww, seed)
        _REFS[key] = (maps, images, idx, OC.reference(maps, images, idx, OC.viridis(), blur))
    return _REFS[key]


def raw_overlay(maps, images, idx, lut, flags, gamma=OC.GAMMA, vmin=0.0, vmax=0.0, want=("f32", "u8", "map"), workspace_bytes=None,
                overrides=None, expect=0):
    """cvcl_attn_overlay through ctypes, twice, on canary-filled outputs -> (rc, {name: numpy}); asserts the two runs agree bit for
    bit.  ``overrides``: raw argument replacements for the refusal tests (then nothing may be written)."""
    H, lib = _lib()
    dev = torch.device("cuda:0")
    N, _, Hh, Ww = images.shape
    M, h, w = maps.shape
    d_maps, d_img = maps.float().contiguous().to(dev), images.float().contiguous().to(dev)
    d_idx = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    d_lut = torch.as_tensor(np.asarray(lut, dtype=np.float32)).to(dev)
    a = dict(maps=H.ptr(d_maps), M=M, h=h, w=w, images=H.ptr(d_img), N=N, H=Hh, W=Ww, idx=H.ptr(d_idx), lut=H.ptr(d_lut), n_lut=d_lut.shape[0],
             flags=flags, f32=True, u8=True, map=True)
    a.update(overrides or {})
    need = lib.cvcl_attn_overlay_workspace_bytes(M, h, w, Hh, Ww, flags)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    mean_c, std_c = (ctypes.c_float * 3)(*OC.MEAN), (ctypes.c_float * 3)(*OC.STD)
    runs = []
    for _ in range(2):
        o_f32 = torch.full((M, Hh, Ww, 3), CANARY_F, dtype=torch.float32, device=dev)
        o_u8 = torch.full((M, Hh, Ww, 3), CANARY_U8, dtype=torch.uint8, device=dev)
        o_map = torch.full((M, Hh, Ww), CANARY_F, dtype=torch.float32, device=dev)
        rc = lib.cvcl_attn_overlay(a["maps"], a["M"], a["h"], a["w"], a["images"], a["N"], a["H"], a["W"], ctypes.cast(mean_c, ctypes.c_void_p),
                                   ctypes.cast(std_c, ctypes.c_void_p), a["idx"], a["lut"], a["n_lut"], a["flags"], gamma, vmin, vmax, None,
                                   3 * Ww, M * Hh * Ww * 3, H.ptr(o_f32) if "f32" in want and a["f32"] else None,
                                   H.ptr(o_u8) if "u8" in want and a["u8"] else None, H.ptr(o_map) if "map" in want and a["map"] else None,
                                   H.ptr(ws), need if workspace_bytes is None else workspace_bytes, H.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect, (rc, lib.cvcl_last_error())
        runs.append({"f32": o_f32.cpu().numpy(), "u8": o_u8.cpu().numpy(), "map": o_map.cpu().numpy()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), f"{k}: two runs differ"
        if expect != 0 or k not in want:
            assert (runs[0][k] == (CANARY_U8 if k == "u8" else CANARY_F)).all(), f"{k}: written to although not asked for / refused"
    return rc, runs[0]


def _no_canary(res):
    assert not (res["f32"] == CANARY_F).any() and not (res["map"] == CANARY_F).any(), "a pixel was not written"


@pytest.mark.parametrize("name", list(OC.CASES))
def test_blurred_overlay_against_float64(name):
    """every case of the table with the blur: out_map, out_f32 and out_u8 within the bounds"""
    from multimodal import _hip as H
    maps, images, idx, ref = _ref(name, True)
    _, res = raw_overlay(maps, images, idx, OC.viridis(), H.OVERLAY_BLUR)
    _no_canary(res)
    OC.check_against_reference(ref, OC.viridis(), res["map"], res["f32"], res["u8"], label=name)


@pytest.mark.parametrize("name", ["workload_7x7_224", "vit_16x16_64x96"])
def test_unblurred_overlay_against_float64(name):
    """blur = 0: normalise / colour / blend alone (the min-max pass reads the resized maps)"""
    maps, images, idx, ref = _ref(name, False)
    _, res = raw_overlay(maps, images, idx, OC.viridis(), 0)
    _no_canary(res)
    OC.check_against_reference(ref, OC.viridis(), res["map"], res["f32"], res["u8"], label=name + " (no blur)")


def test_each_output_alone_gives_the_same_bits():
    from multimodal import _hip as H
    maps, images, idx, _ = _ref("odd_3x3_37x53", True)
    _, full = raw_overlay(maps, images, idx, OC.viridis(), H.OVERLAY_BLUR)
    for k in ("f32", "u8", "map"):
        _, one = raw_overlay(maps, images, idx, OC.viridis(), H.OVERLAY_BLUR, want=(k,))
        assert np.array_equal(one[k], full[k])


def _frames_f32(images):
    """img * std + mean in fp32, one multiply and one add: what the kernel computes, bit for bit -> [N, H, W, 3]"""
    std = torch.tensor(OC.STD, dtype=torch.float32).view(1, 3, 1, 1)
    mean = torch.tensor(OC.MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    return (images.float() * std + mean).permute(0, 2, 3, 1).contiguous()


def _u8_of(frames):
    return torch.floor(frames.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).numpy()


@pytest.mark.parametrize("kind", ["zeros_resized", "constant_unresized"])
def test_constant_map_leaves_the_frame(kind):
    """A map without a range has x = m - lo = 0 everywhere: out_map is exactly 0 and the output is exactly the de-normalised frame.
    All-zero maps (a Grad-CAM with nothing positive) through the resize and the blur; a constant 0.25 without the resize (a resized
    constant is constant only up to the rounding of the cubic weights, in float64 as well)."""
    from multimodal import _hip as H
    if kind == "zeros_resized":
        maps, images = torch.zeros(2, 7, 7), OC.make_images(2, 224, 224, 3, overshoot=0.1)
    else:
        maps, images = torch.full((1, 8, 200), 0.25), OC.make_images(1, 8, 200, 4, overshoot=0.1)
    _, res = raw_overlay(maps, images, None, OC.viridis(), H.OVERLAY_BLUR)
    frames = _frames_f32(images)
    assert (res["map"] == 0.0).all()
    assert np.array_equal(res["f32"], frames.numpy())
    assert np.array_equal(res["u8"], _u8_of(frames))
    assert res["u8"].min() == 0 and res["u8"].max() == 255                   # both clamps were met


def test_given_range_clamps():
    """vmin / vmax inside the map's range: x is clamped to [0, 1] and nothing is NaN (getAttMap's x ** 0.7 is NaN below vmin); the
    reference with the same clamp"""
    from multimodal import _hip as H
    name = "vit_16x16_64x96"
    maps, images, idx, plain = _ref(name, True)
    lo, hi = max(plain["lo"]), min(plain["hi"])                             # inside every map's own range
    vmin, vmax = float(np.float32(lo + 0.3 * (hi - lo))), float(np.float32(lo + 0.7 * (hi - lo)))
    ref = OC.reference(maps, images, idx, OC.viridis(), True, vmin=vmin, vmax=vmax)
    assert (ref["x"] == 0).any() and (ref["x"] == 1).any()
    _, res = raw_overlay(maps, images, idx, OC.viridis(), H.OVERLAY_BLUR | H.OVERLAY_HAS_RANGE, vmin=vmin, vmax=vmax)
    _no_canary(res)
    assert res["map"].min() == 0.0 and res["map"].max() == 1.0
    OC.check_against_reference(ref, OC.viridis(), res["map"], res["f32"], res["u8"], label=name + " (given range)")


@pytest.mark.parametrize("n_lut", [2, 1024])
def test_table_sizes(n_lut):
    """the smallest and the largest colour table (a smooth ramp: the adjacent step shrinks with the size)"""
    from multimodal import _hip as H
    name = "odd_3x3_37x53"
    maps, images, idx, _ = _ref(name, True)
    t = np.linspace(0.0, 1.0, n_lut)
    lut = np.stack([t, 1.0 - t, 0.5 + 0.5 * np.sin(3.0 * t)], 1).astype(np.float32)
    ref = OC.reference(maps, images, idx, lut, True)
    _, res = raw_overlay(maps, images, idx, lut, H.OVERLAY_BLUR)
    OC.check_against_reference(ref, lut, res["map"], res["f32"], res["u8"], label=f"{name} ({n_lut} entries)")


def test_refusals_leave_the_outputs_alone():
    """H = 1025, h > H, n_lut = 1, no output pointer, null maps, a workspace that is too small: CVCL_EINVAL, canaries intact"""
    from multimodal import _hip as H
    maps, images, idx, _ = _ref("odd_3x3_37x53", True)
    lut, f = OC.viridis(), H.OVERLAY_BLUR
    for overrides in (dict(H=1025), dict(h=38), dict(n_lut=1), dict(f32=False, u8=False, map=False), dict(maps=None), dict(flags=64)):
        raw_overlay(maps, images, idx, lut, f, overrides=overrides, expect=EINVAL)
    need = H.lib().cvcl_attn_overlay_workspace_bytes(5, 3, 3, 37, 53, f)
    raw_overlay(maps, images, idx, lut, f, workspace_bytes=need - 1, expect=EINVAL)
    assert b"workspace" in H.lib().cvcl_last_error()


def test_python_entry_layouts():
    """overlay_attention_maps: [M, h, w] with image_index, [N, k, h, w] and [N, 1, h, w] maps, out = "both", return_map, an explicit
    table -- the bits of the raw entry, in the maps' leading shape"""
    from multimodal import _hip as H
    from multimodal.attention_maps import overlay_attention_maps
    dev = torch.device("cuda:0")
    maps, images, idx, _ = _ref("odd_3x3_37x53", True)
    _, raw = raw_overlay(maps, images, idx, OC.viridis(), H.OVERLAY_BLUR)
    f32, u8, x = overlay_attention_maps(images.to(dev), maps.to(dev), image_index=idx, out="both", return_map=True)
    assert f32.shape == (5, 37, 53, 3) and u8.dtype == torch.uint8 and x.shape == (5, 37, 53)
    assert np.array_equal(f32.cpu().numpy(), raw["f32"]) and np.array_equal(u8.cpu().numpy(), raw["u8"]) and np.array_equal(x.cpu().numpy(), raw["map"])
    # image n with its k = 2 maps; the same through an explicit table and an explicit index
    block = overlay_attention_maps(images.to(dev), maps[:4].view(2, 2, 3, 3).to(dev), cmap=OC.viridis())
    flat = overlay_attention_maps(images.to(dev), maps[:4].to(dev), image_index=torch.tensor([0, 0, 1, 1], device=dev))
    assert block.shape == (2, 2, 37, 53, 3) and torch.equal(block.view(4, 37, 53, 3), flat)
    single = overlay_attention_maps(images.to(dev), maps[:2, None].to(dev), out="float")
    assert single.shape == (2, 1, 37, 53, 3) and single.dtype == torch.float32
    with pytest.raises(ValueError):
        overlay_attention_maps(images.to(dev), maps.to(dev))                  # 5 maps, 2 images, no index
    with pytest.raises(ValueError):
        overlay_attention_maps(images.to(dev), maps.to(dev), image_index=[0, 0, 1, 1, 2])
    with pytest.raises(H.CvclError):
        overlay_attention_maps(images, maps[:2])                             # CPU tensors


@pytest.mark.parametrize("K,nrow", [(3, 2), (8, 4)])
def test_attention_grid_is_make_grid_of_the_tiles(K, nrow):
    """the canvas equals the frames and the overlays pasted with numpy at torchvision.utils.make_grid's offsets, bit for bit (K = 3,
    nrow = 2: a ragged last row; the canvas rows are not 4-byte multiples: the unaligned store path)"""
    from multimodal.attention_maps import attention_grid, overlay_attention_maps
    dev = torch.device("cuda:0")
    Hh, Ww, pad = 20, 28, 2
    maps, images = OC.make_maps(K, 5, 5, 7), OC.make_images(K, Hh, Ww, 7, overshoot=0.1)
    canvas = attention_grid(images.to(dev), maps.to(dev), nrow=nrow, padding=pad)
    again = attention_grid(images.to(dev), maps[:, None].to(dev), nrow=nrow, padding=pad)
    assert torch.equal(canvas, again)
    tiles = np.concatenate([_u8_of(_frames_f32(images)), overlay_attention_maps(images.to(dev), maps.to(dev)).cpu().numpy()])
    xmaps = min(nrow, 2 * K)
    ymaps = math.ceil(2 * K / xmaps)
    want = np.zeros(((Hh + pad) * ymaps + pad, (Ww + pad) * xmaps + pad, 3), dtype=np.uint8)
    for k, tile in enumerate(tiles):
        y, x = (k // xmaps) * (Hh + pad) + pad, (k % xmaps) * (Ww + pad) + pad
        want[y:y + Hh, x:x + Ww] = tile
    assert canvas.shape == want.shape and np.array_equal(canvas.cpu().numpy(), want)


def _child(argv, cwd, seconds):
    """a fresh process under its own time limit"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "multimodal-baby_amd")]))
    r = subprocess.run([sys.executable] + argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_generate_attention_maps_script(tmp_path):
    """generate_attention_maps.py --synthetic: one JPEG per class, sized as make_grid sizes 2 K tiles of 224 x 224"""
    from PIL import Image
    from multimodal.alignment import SYNTHETIC_WORDS
    from multimodal.attention_maps import grid_geometry
    out = tmp_path / "figures"
    _child([os.path.join(ROOT, "generate_attention_maps.py"), "--synthetic", "--num_samples_per_class", "3", "--nrow", "2", "--out_dir", str(out)],
           str(tmp_path), 240)
    Hc, Wc, _ = grid_geometry(6, 224, 224, 2, 2)
    for word in SYNTHETIC_WORDS:
        with Image.open(out / f"{word}.jpg") as im:
            assert im.size == (Wc, Hc) and im.mode == "RGB"
            a = np.asarray(im)
        assert a[:2].mean() < 32 and a[2:226, 2:226].max() > 64               # the padding is (JPEG-)black, the first frame is not


def test_eval_entry_attention_overlays(dev, tmp_path, monkeypatch):
    """eval.py --eval_dataset synthetic --attention_overlays in a child process: one PNG per trial at the frames' size, and trial 0's
    PNG within the uint8 bounds of getAttMap applied to the same frame and map (the map eval.py saved beside it)."""
    import train
    from PIL import Image
    from multimodal.attention_maps import getAttMap
    from multimodal.multimodal_data_module import SyntheticEvalTrials
    monkeypatch.chdir(tmp_path)
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features "
            f"--checkpoint_callback True --logger False --exp_name {exp}").split()
    with contextlib.redirect_stdout(io.StringIO()):
        train.main(argv)
    d = tmp_path / "overlays"
    _child([os.path.join(ROOT, "eval.py"), "--checkpoint", exp, "--eval_dataset", "synthetic", "--n_trials", "4", "--trial_batch", "4",
            "--attention_overlays", "--attention_maps", str(d)], str(tmp_path), 240)
    pngs = sorted(d.glob("*_attn_map.png"))
    assert len(pngs) == 4
    imgs, _label, _n, _ = SyntheticEvalTrials(4, 2350, seed=0 + 4, eval_type="image")[0]
    frame = imgs[0].float()
    size = tuple(frame.shape[1:])
    for p in pngs:
        with Image.open(p) as im:
            assert im.size == (size[1], size[0]) and im.mode == "RGB"
    cam = torch.from_numpy(np.load(d / "cams.npy")[0, 0])
    att = torch.nn.functional.interpolate(cam.double()[None, None], size=size, mode="bicubic", align_corners=False)[0, 0].numpy()
    img = OC.frames64(frame[None])[0]
    with contextlib.redirect_stdout(io.StringIO()):
        want = getAttMap(img, att)                                           # float64: scipy's blur, matplotlib's viridis, the 0.7 blend
    want_u8 = np.floor(np.clip(want, 0, 1) * 255 + 0.5).astype(np.int64)
    (first,) = [p for p in pngs if p.name.endswith("_0_attn_map.png")]
    with Image.open(first) as im:
        got = np.asarray(im).astype(np.int64)
    ref = OC.reference(cam[None], frame[None], None, OC.viridis(), True)
    assert np.array_equal(ref["u8"][0], want_u8)                             # overlay_common's restatement IS getAttMap
    diff = np.abs(got - want_u8).max(-1)
    near, step = ref["near"][0], OC.lut_step(OC.viridis())
    print(f"eval overlay: near-edge share {near.mean():.4%}, max count off the edges {diff[~near].max()}, on them {diff[near].max() if near.any() else 0}")
    assert near.mean() <= OC.share_limit(256)
    assert diff[~near].max() <= 1 and (not near.any() or diff[near].max() <= 1 + math.ceil(255 * step))
