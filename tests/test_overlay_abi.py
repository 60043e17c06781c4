"""CPU: the attention-overlay entries of the C ABI (cvcl_attn_overlay, cvcl_attn_overlay_workspace_bytes) are exported and refuse bad
arguments with CVCL_EINVAL before any launch; the workspace query grows with M H W; colour tables resolve and are cached; the grid
geometry is torchvision.utils.make_grid's; the figure script's and eval.py's argument parsers know the new options."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

EINVAL = -1


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    _hip.load()
    return _hip


def test_entries_refuse_bad_arguments_before_any_launch(H):
    l = H.lib()
    d = 16                                                    # aligned non-null stand-in: validation never dereferences
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    host = ctypes.cast(three, ctypes.c_void_p)
    ok = dict(maps=d, M=2, h=7, w=7, images=d, N=2, H=224, W=224, mean=host, std=host, idx=None, lut=d, n_lut=256, flags=H.OVERLAY_BLUR,
              gamma=0.7, vmin=0.0, vmax=0.0, dst=None, pitch=3 * 224, elems=2 * 224 * 224 * 3, f32=d, u8=None, map=None, ws=d, ws_bytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return l.cvcl_attn_overlay(a["maps"], a["M"], a["h"], a["w"], a["images"], a["N"], a["H"], a["W"], a["mean"], a["std"], a["idx"],
                                   a["lut"], a["n_lut"], a["flags"], a["gamma"], a["vmin"], a["vmax"], a["dst"], a["pitch"], a["elems"],
                                   a["f32"], a["u8"], a["map"], a["ws"], a["ws_bytes"], None)

    def err():
        return l.cvcl_last_error()

    for bad in (dict(H=1025), dict(W=1025), dict(H=0)):
        assert call(**bad) == EINVAL and b"output size" in err()
    for bad in (dict(h=225), dict(w=225), dict(h=0)):
        assert call(**bad) == EINVAL and b"map size" in err()
    for bad in (dict(n_lut=1), dict(n_lut=1025)):
        assert call(**bad) == EINVAL and b"n_lut" in err()
    assert call(f32=None) == EINVAL and b"no output" in err()
    for bad in (dict(maps=None), dict(lut=None), dict(images=None), dict(mean=None), dict(std=None)):
        assert call(**bad) == EINVAL and b"null" in err()
    assert call(ws_bytes=1024) == EINVAL and b"workspace" in err()
    assert call(ws=None) == EINVAL and b"workspace" in err()
    assert call(M=0) == EINVAL and call(N=0) == EINVAL
    assert call(M=3) == EINVAL and b"image_of_map" in err()                       # map 2 has no image 2
    assert call(flags=8) == EINVAL and b"flags" in err()
    assert call(gamma=-1.0) == EINVAL and call(gamma=float("nan")) == EINVAL and b"gamma" in err()
    assert call(flags=H.OVERLAY_HAS_RANGE, vmin=float("nan")) == EINVAL
    assert call(pitch=3 * 224 - 1) == EINVAL and b"row_pitch" in err()
    assert call(elems=2 * 224 * 224 * 3 - 1) == EINVAL and b"out_elems" in err()
    assert call(maps=d + 4) == EINVAL and b"aligned" in err()
    # the frames-only form needs neither maps nor a table, but still an image, an output and room for it
    assert call(flags=H.OVERLAY_IMAGE_ONLY, maps=None, lut=None, n_lut=0, f32=None, map=d) == EINVAL and b"no output" in err()


def test_workspace_query(H):
    q = H.lib().cvcl_attn_overlay_workspace_bytes
    f = H.OVERLAY_BLUR
    sizes = [(1, 1, 1), (1, 37, 53), (2, 64, 96), (2, 224, 224), (5, 224, 224), (1024, 224, 224), (3, 1024, 1024)]
    sizes.sort(key=lambda s: s[0] * s[1] * s[2])
    got = [q(M, 1, 1, Hh, Ww, f) for M, Hh, Ww in sizes]
    assert all(g > 0 for g in got) and got == sorted(got)                          # monotone in M H W
    assert q(2, 7, 7, 224, 224, f) >= 2 * 2 * 224 * 224 * 4                        # two fp32 planes: the two filter passes
    assert q(2, 7, 7, 224, 224, 0) >= 2 * 224 * 224 * 4 > q(2, 224, 224, 224, 224, 0) > 0       # the resized maps; nothing but partials
    assert q(2, 7, 7, 224, 224, H.OVERLAY_IMAGE_ONLY) < 1024
    for bad in ((0, 7, 7, 224, 224, f), (2, 7, 7, 1025, 224, f), (2, 225, 7, 224, 224, f), (2, 7, 7, 224, 224, 8)):
        assert q(*bad) == 0


def test_colour_tables_resolve_and_are_cached():
    from multimodal import attention_maps as A
    from multimodal.colormaps import VIRIDIS
    lut = A.resolve_lut("viridis")                                                  # built in: no matplotlib needed
    assert lut.dtype == np.float32 and lut.shape == (256, 3) and np.array_equal(lut, np.asarray(VIRIDIS, dtype=np.float32))
    matplotlib = pytest.importorskip("matplotlib")
    for name in ("viridis", "magma", "Greys_r"):
        cm = matplotlib.colormaps[name]
        assert np.array_equal(A.resolve_lut(name), cm(np.arange(cm.N))[:, :3].astype(np.float32)), name
    own = np.linspace(0, 1, 12).reshape(4, 3)
    assert np.array_equal(A.resolve_lut(own), own.astype(np.float32)) and np.array_equal(A.resolve_lut(torch.from_numpy(own)), own.astype(np.float32))
    for bad in (np.zeros((1, 3)), np.zeros((1025, 3)), np.zeros((4, 4)), np.zeros(6)):
        with pytest.raises(ValueError):
            A.resolve_lut(bad)
    a, b = A.device_lut("magma", "cpu"), A.device_lut("magma", "cpu")
    assert a is b and a.shape == (256, 3)                                           # one upload per (name, device)
    assert A.device_lut(own, "cpu") is not A.device_lut(own, "cpu")                 # explicit tables are the caller's to keep


def test_grid_geometry_is_make_grid():
    """torchvision.utils.make_grid: xmaps = min(nrow, n), ymaps = ceil(n / xmaps), cells of (H + p) x (W + p), a canvas of
    (H + p) ymaps + p by (W + p) xmaps + p, tile k at ((k // xmaps) (H + p) + p, (k % xmaps) (W + p) + p)"""
    from multimodal.attention_maps import grid_geometry
    assert grid_geometry(16, 224, 224, 4, 2) == (4 * 226 + 2, 4 * 226 + 2, [(2 + 226 * (k // 4), 2 + 226 * (k % 4)) for k in range(16)])
    Hc, Wc, at = grid_geometry(6, 20, 28, 2, 2)                                    # K = 3, nrow = 2: three rows of two
    assert (Hc, Wc) == (68, 62) and at == [(2, 2), (2, 32), (24, 2), (24, 32), (46, 2), (46, 32)]
    Hc, Wc, at = grid_geometry(3, 5, 7, 8, 1)                                      # fewer tiles than nrow: one row of three
    assert (Hc, Wc) == (7, 25) and at == [(1, 1), (1, 9), (1, 17)]
    assert grid_geometry(5, 4, 4, 2, 0) == (12, 8, [(0, 0), (0, 4), (4, 0), (4, 4), (8, 0)])     # a ragged last row
    for bad in ((0, 4, 4, 2, 2), (4, 4, 4, 0, 2), (4, 4, 4, 2, -1)):
        with pytest.raises(ValueError):
            grid_geometry(*bad)


def test_python_entries_refuse_cpu_tensors(H):
    from multimodal.attention_maps import attention_grid, overlay_attention_maps
    with pytest.raises(H.CvclError):
        overlay_attention_maps(torch.randn(2, 3, 8, 8), torch.rand(2, 4, 4))
    with pytest.raises(H.CvclError):
        attention_grid(torch.randn(2, 3, 8, 8), torch.rand(2, 4, 4))


def test_figure_script_arguments_and_selection():
    import random
    import generate_attention_maps as G
    a = G.parser().parse_args([])
    assert (a.num_samples_per_class, a.nrow, a.seed, a.precision) == (8, 4, 0, "32") and not a.synthetic and not a.use_kitty_label
    a = G.parser().parse_args("--checkpoint c.ckpt --data_dir d --num_samples_per_class 4 --nrow 2 --seed 3 --use_kitty_label --out_dir o "
                              "--precision bf16".split())
    assert (a.checkpoint, a.data_dir, a.num_samples_per_class, a.nrow, a.seed, a.out_dir, a.precision) == ("c.ckpt", "d", 4, 2, 3, "o", "bf16")
    G.check_args(a)
    G.check_args(G.parser().parse_args(["--synthetic"]))
    for argv in ([], ["--checkpoint", "c.ckpt"], ["--data_dir", "d"], ["--synthetic", "--data_dir", "d"], ["--synthetic", "--nrow", "0"]):
        with pytest.raises(SystemExit):
            G.check_args(G.parser().parse_args(argv))
    # the reference's selection: random.seed(seed), every class's index list shuffled in class order, the first n kept
    targets = [0] * 5 + [1] * 3 + [2] * 6
    random.seed(0)
    lists = {0: list(range(5)), 1: list(range(5, 8)), 2: list(range(8, 14))}
    for c in lists:
        random.shuffle(lists[c])
    assert G.select_per_class(targets, 3, 4, seed=0) == {c: v[:4] for c, v in lists.items()}
    assert G.select_per_class(targets, 3, 4, seed=1) != G.select_per_class(targets, 3, 4, seed=0)


def test_eval_flag_and_its_clip_refusal():
    import eval as ev
    args = ev._parser().parse_args(["--eval_dataset", "synthetic", "--attention_overlays"])
    assert args.attention_overlays and not args.plot_attention
    assert not ev._parser().parse_args([]).attention_overlays
    clip = ev._parser().parse_args(["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "bpe.txt", "--attention_overlays"])
    with pytest.raises(SystemExit, match="--attention_overlays is not built for --clip_eval"):
        ev.check_clip_args(clip)
    ev.check_clip_args(ev._parser().parse_args(["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "bpe.txt"]))
