"""GPU: cvcl_preprocess_frames (csrc/preprocess.hip through multimodal.preprocess.DevicePreprocess) against the Pillow golden fixture
and the numpy restatement of Pillow's bicubic resize (tests/preprocess_common.py) -- every comparison is equality, on the uint8 image
and on the fp32 normalised tensor."""
import zlib

import numpy as np
import pytest
import torch

import preprocess_common as P
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZE = 224
# H x W of the ragged batch: identity, down, up, one pass barely down and one barely up, tiny, one pass 5x down and one 4x up,
# a source that the centre crop does not resize, and the reference's frame size in both orientations
SMALL = [(224, 224), (240, 320), (100, 75), (225, 223), (7, 5), (300, 60), (224, 301), (480, 640), (640, 480)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def small_frames():
    return [P.case_frame(40 + i, h, w, (0, 1, 4)[i % 3]) for i, (h, w) in enumerate(SMALL)]


def _pre(mode, **kw):
    from multimodal.preprocess import DevicePreprocess
    mean, std = P.mode_stats(mode)
    return DevicePreprocess(size=SIZE, mode=mode, mean=mean, std=std, **kw)


def _run(frames, mode):
    out, out8 = _pre(mode)(frames, return_uint8=True)
    return out.cpu().numpy(), out8.cpu().numpy()


def _want(frame, mode):
    from multimodal.preprocess import resize_geometry
    u8 = P.resize_window_u8(frame, *resize_geometry(frame.shape[0], frame.shape[1], SIZE, mode), SIZE, SIZE)
    return P.to_tensor_normalize(u8, *P.mode_stats(mode)), u8


def test_pillow_golden_bit_exact(dev):
    from multimodal.preprocess import MODES
    g = np.load(GOLDEN + "/preprocess_pil.npz")
    for i in range(int(g["n_cases"])):
        H, W, mode, cell, seed = (int(v) for v in g[f"case{i}"])
        mode = MODES[mode]
        out, out8 = _run([P.case_frame(seed, H, W, cell)], mode)
        assert zlib.crc32(out8[0].tobytes()) == int(g[f"u8_crc{i}"]), f"case {i}"
        if f"u8_{i}" in g.files:
            assert np.array_equal(out8[0], g[f"u8_{i}"])
        if f"tensor{i}_rows0_16" in g.files:
            assert np.array_equal(out[0][:, :16], g[f"tensor{i}_rows0_16"])
        assert np.array_equal(out[0], P.to_tensor_normalize(out8[0], *P.mode_stats(mode)))      # fp32 of every case, bit for bit


@pytest.mark.parametrize("mode", ["stretch", "shorter_side_center_crop"])
def test_ragged_batch_vs_restatement_bit_exact(dev, small_frames, mode):
    out, out8 = _run(small_frames, mode)
    assert out.shape == (len(SMALL), 3, SIZE, SIZE) and out8.shape == (len(SMALL), SIZE, SIZE, 3)
    for i, frame in enumerate(small_frames):
        want, want8 = _want(frame, mode)
        assert np.array_equal(out8[i], want8), (i, SMALL[i])
        assert np.array_equal(out[i], want), (i, SMALL[i])
    again, again8 = _run(small_frames, mode)                                   # two runs, identical results
    assert np.array_equal(out, again) and np.array_equal(out8, again8)


@pytest.mark.parametrize("mode,cell", [("stretch", 0), ("shorter_side_center_crop", 24)])
def test_full_hd_frame_vs_restatement(dev, mode, cell):
    """1080 x 1920: 35 / 21 taps per output index, a tile of 170 source rows per band"""
    frame = P.case_frame(90, 1080, 1920, cell)
    out, out8 = _run([frame], mode)
    want, want8 = _want(frame, mode)
    assert np.array_equal(out8[0], want8)
    assert np.array_equal(out[0], want)


def test_identity_is_totensor_normalize(dev):
    from multimodal.preprocess import DevicePreprocess, IMAGENET_MEAN, IMAGENET_STD
    frames = torch.randint(0, 256, (5, SIZE, SIZE, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    want = (frames.permute(0, 3, 1, 2).float().div(255) - mean) / std          # torch's CPU (IEEE) ops
    for mode in ("stretch", "shorter_side_center_crop"):
        got, got8 = DevicePreprocess(mode=mode)(frames.to(dev), return_uint8=True)
        assert torch.equal(got.cpu(), want) and torch.equal(got8.cpu(), frames)


def test_input_forms_agree(dev):
    """a list of numpy arrays, a list of device tensors, the packed [B, H, W, 3] tensor (host and device) and single images"""
    pre = _pre("shorter_side_center_crop")
    frames = np.stack([P.case_frame(60 + i, 120, 90, i % 2) for i in range(4)])
    ref, ref8 = pre(list(frames), return_uint8=True)
    assert ref.is_cuda and ref.dtype == torch.float32 and ref8.dtype == torch.uint8
    for form in (torch.from_numpy(frames), torch.from_numpy(frames).to(dev), [torch.from_numpy(f).to(dev) for f in frames],
                 [frames[0], torch.from_numpy(frames[1]).to(dev), frames[2], torch.from_numpy(frames[3])]):
        out, out8 = pre(form, return_uint8=True)
        assert torch.equal(out, ref) and torch.equal(out8, ref8)
    one = pre(frames[2])
    assert one.shape == (3, SIZE, SIZE) and torch.equal(one, ref[2])
    assert pre(frames[2]).unsqueeze(0).shape == (1, 3, SIZE, SIZE)             # the reference's preprocess(img).unsqueeze(0)
    one, one8 = pre(torch.from_numpy(frames[1]), return_uint8=True)
    assert torch.equal(one, ref[1]) and one8.shape == (SIZE, SIZE, 3) and torch.equal(one8, ref8[1])


def test_pil_image_input(dev):
    Image = pytest.importorskip("PIL.Image")
    frame = P.case_frame(70, 50, 80, 0)
    pre = _pre("stretch")
    assert torch.equal(pre(Image.fromarray(frame)), pre(frame))
    grey = Image.fromarray(frame[:, :, 0])                                      # any mode goes through convert("RGB")
    assert torch.equal(pre(grey), pre(np.repeat(frame[:, :, :1], 3, axis=2)))


def test_alignment_resize_end_to_end(dev, tmp_path):
    """alignment.py --resize runs end to end on a folder of mixed-size PNGs, which the stored-size path refuses"""
    Image = pytest.importorskip("PIL.Image")
    from multimodal import alignment as A
    from multimodal import neighbors as NB
    words, sizes = ("ball", "car", "dog"), [(48, 64), (64, 48), (37, 91), (224, 224)]
    for c, word in enumerate(words):
        (tmp_path / "eval" / word).mkdir(parents=True)
        for j, (h, w) in enumerate(sizes):
            Image.fromarray(P.case_frame(100 + 10 * c + j, h, w, 0)).save(tmp_path / "eval" / word / f"img_{j}.png")
    with pytest.raises(ValueError, match="different sizes"):                   # the stored-size path still refuses the folder
        NB.load_folder_u8(str(tmp_path / "eval"))
    frames, labels, names = NB.load_folder_list_u8(str(tmp_path / "eval"))
    assert len(frames) == 12 and sorted(set(labels)) == list(words) and {tuple(f.shape) for f in frames} == {(h, w, 3) for h, w in sizes}
    args = A.parser().parse_args(["--eval_dir", str(tmp_path / "eval"), "--random_init", "--resize", "--no_replace", "--batch_size", "5",
                                  "--out", str(tmp_path / "out")])
    assert not A.parser().parse_args([]).resize                                 # off by default
    summary = A.main(args)
    feats = np.load(tmp_path / "out" / "cvc_all_image_features_seed_0.npy")
    assert feats.shape == (12, 512) and np.isfinite(feats).all() and set(summary["paired_distances"]) == set(words)
