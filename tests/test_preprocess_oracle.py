"""CPU: the numpy restatement of the evaluation-time transform (tests/preprocess_common.py) against the Pillow golden fixture
(tests/golden/preprocess_pil.npz, written by Pillow itself: tools/gen_golden_preprocess.py) and, where Pillow is importable, against
the live library on random sizes and windows -- all bit for bit -- and the host geometry rules against their literal cases."""
import zlib

import numpy as np
import pytest

import preprocess_common as P
from conftest import GOLDEN

SIZE = 224


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN + "/preprocess_pil.npz")


def _modes():
    from multimodal.preprocess import MODES
    return MODES


def test_restatement_equals_pillow_golden(g):
    from multimodal.preprocess import resize_geometry
    assert int(g["size"]) == SIZE
    shapes, hard = set(), 0
    for i in range(int(g["n_cases"])):
        H, W, mode, cell, seed = (int(v) for v in g[f"case{i}"])
        mode = _modes()[mode]
        frame = P.case_frame(seed, H, W, cell)
        assert zlib.crc32(frame.tobytes()) == int(g[f"frame_crc{i}"]), f"case {i}: input"
        geom = tuple(int(v) for v in g[f"geometry{i}"])
        assert resize_geometry(H, W, SIZE, mode) == geom, f"case {i}: geometry"
        u8 = P.resize_window_u8(frame, *geom, SIZE, SIZE)
        assert zlib.crc32(u8.tobytes()) == int(g[f"u8_crc{i}"]), f"case {i}"
        if f"u8_{i}" in g.files:
            assert np.array_equal(u8, g[f"u8_{i}"])
        if f"tensor{i}_rows0_16" in g.files:
            assert np.array_equal(P.to_tensor_normalize(u8, *P.mode_stats(mode))[:, :16], g[f"tensor{i}_rows0_16"])
        if cell:
            hard += 1
            assert (u8 == 0).any() and (u8 == 255).any()                      # the clamp of the passes is exercised on both sides
        shapes.add((H, W, mode))
    assert hard >= 6
    assert sum(f"u8_{i}" in g.files for i in range(int(g["n_cases"]))) == 2
    for need in [(224, 224, "stretch"), (240, 320, "stretch"), (100, 75, "stretch"), (225, 223, "stretch"), (7, 5, "stretch"),
                 (300, 60, "stretch"), (480, 640, "stretch"), (480, 640, "shorter_side_center_crop"),
                 (640, 480, "shorter_side_center_crop"), (1080, 1920, "stretch"), (1080, 1920, "shorter_side_center_crop")]:
        assert need in shapes, need


def test_restatement_equals_live_pillow():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    assert PIL.__version__
    rng = np.random.default_rng(7)
    for i in range(24):
        H, W = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        rh, rw = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        if i % 6 == 0:
            rh = H                                                            # a skipped pass
        if i % 8 == 1:
            rw = W
        oh, ow = int(rng.integers(1, rh + 1)), int(rng.integers(1, rw + 1))
        ct, cl = int(rng.integers(0, rh - oh + 1)), int(rng.integers(0, rw - ow + 1))
        frame = P.case_frame(300 + i, H, W, (0, 1, 5)[i % 3])
        want = np.asarray(Image.fromarray(frame).resize((rw, rh), Image.BICUBIC).crop((cl, ct, cl + ow, ct + oh)))
        got = P.resize_window_u8(frame, rh, rw, ct, cl, oh, ow)
        assert np.array_equal(got, want), (i, H, W, rh, rw, ct, cl, oh, ow)


@pytest.mark.parametrize("w,h,rw,rh,cl,ct", [
    (640, 480, 298, 224, 37, 0),
    (480, 640, 224, 298, 0, 37),
    (500, 333, 336, 224, 56, 0),
    (301, 224, 301, 224, 38, 0),              # no resize; 38.5 rounds to the even 38
    (303, 224, 303, 224, 40, 0),              # 39.5 rounds to the even 40
    (224, 224, 224, 224, 0, 0),
])
def test_center_crop_geometry_literals(w, h, rw, rh, cl, ct):
    from multimodal.preprocess import resize_geometry
    assert resize_geometry(h, w, SIZE, "shorter_side_center_crop") == (rh, rw, ct, cl)


def test_stretch_geometry_and_unknown_mode():
    from multimodal.preprocess import DevicePreprocess, resize_geometry
    assert resize_geometry(480, 640, SIZE, "stretch") == (224, 224, 0, 0)
    assert resize_geometry(7, 5, 96, "stretch") == (96, 96, 0, 0)
    with pytest.raises(ValueError, match="mode"):
        resize_geometry(10, 10, SIZE, "pad")
    with pytest.raises(ValueError, match="mode"):
        DevicePreprocess(mode="pad")
