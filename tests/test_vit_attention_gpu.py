"""GPU: the ViT's self-attention maps and intermediate layers (csrc/vit_maps.hip, multimodal/vit_maps.py) against float64.

Bounds.  Kernel and full-size tests: tau = 4 x the worst absolute error of torch's own fp32 CPU evaluation of the same expression
against float64 on the same inputs, computed inside the test (the rule of tests/test_neighbors_gpu.py; the 4 covers a different but
equally valid summation order).  Goldens: 2e-5 relative, the bound tests/test_encoders_gpu.py holds the ViT forward to.  bf16 maps:
2 x the deviation of torch CPU autocast(bfloat16) from its own fp32 run on the same weights and batch (the kernel rounds qkv once
more than autocast does).  Every case prints its bound and the measured error before it asserts."""
import contextlib
import functools
import io
import json
from functools import partial

import numpy as np
import pytest
import torch

import vit_attention_common as VC
from conftest import load_golden, maxrel

pytestmark = pytest.mark.gpu

SHAPES = [(4, 12, 197, 64), (2, 12, 257, 64), (1, 6, 785, 64), (3, 3, 33, 64), (2, 2, 17, 16)]      # (B, heads, T, head_dim)


def _H():
    from multimodal import _hip as H
    return H


def _qkv(B, heads, T, hd, dtype, seed, q_gain=1.0):
    qkv = torch.randn(B, T, 3, heads, hd, generator=torch.Generator().manual_seed(seed))
    qkv[:, :, 0] *= q_gain
    qkv = qkv.reshape(B * T, 3 * heads * hd)
    return qkv.to(dtype).contiguous()                      # bf16: the rounded values ARE the inputs


def _launch(qkv_dev, B, T, heads, hd, scale, q_rows):
    from multimodal import vit_maps
    return vit_maps.attention_probs(qkv_dev, B, T, heads, hd, scale, q_rows)


def _check_kernel(dev, name, qkv, B, heads, T, hd, scale, q_rows_list):
    ref64 = VC.softmax_probs(qkv.double(), B, T, heads, hd, scale)
    ref32 = VC.softmax_probs(qkv.float(), B, T, heads, hd, scale)          # torch's fp32 CPU evaluation of the same inputs
    qd = qkv.to(dev)
    out = []
    for q_rows in q_rows_list:
        tau = VC.tau(ref32[:, :, :q_rows], ref64[:, :, :q_rows])
        got = _launch(qd, B, T, heads, hd, scale, q_rows)
        assert got.shape == (B, heads, q_rows, T) and got.dtype == torch.float32
        err = float((got.double().cpu() - ref64[:, :, :q_rows]).abs().max())               # every element
        rowsum = float((got.double().sum(-1) - 1).abs().max())
        print(f"[probs {name}] B {B} heads {heads} T {T} hd {hd} q_rows {q_rows}: tau {tau:.3e}, kernel error {err:.3e}, "
              f"row sums off 1 by {rowsum:.3e}")
        out.append((q_rows, tau, err, rowsum))
    for q_rows, tau, err, rowsum in out:
        assert err <= tau, (name, q_rows, err, tau)
        assert rowsum <= T * 2.0 ** -23, (name, q_rows, rowsum)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,heads,T,hd", SHAPES)
def test_kernel_vs_float64(dev, dtype, B, heads, T, hd):
    """Random qkv, q_rows in {1, 7, T}, every element compared.  Measured on an MI355X (tau / kernel error at q_rows = T):
    see DESIGN.md section 9 "ViT self-attention maps"."""
    qkv = _qkv(B, heads, T, hd, dtype, seed=T + heads)
    _check_kernel(dev, "f32" if dtype == torch.float32 else "bf16", qkv, B, heads, T, hd, hd ** -0.5, [1, 7, T])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernel_near_one_hot_rows(dev, dtype):
    """Scores scaled so that a row's logits span more than 80: near one-hot rows, far tails flushed to 0."""
    B, heads, T, hd = 2, 12, 197, 64
    qkv = _qkv(B, heads, T, hd, dtype, seed=9, q_gain=20.0)
    q, k, _ = qkv.double().reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    logits = (q @ k.transpose(-2, -1)) * hd ** -0.5
    span = float((logits.max(-1).values - logits.min(-1).values).max())
    assert span > 80, span
    _check_kernel(dev, f"one-hot span {span:.0f}", qkv, B, heads, T, hd, hd ** -0.5, [1, 7, T])


@pytest.mark.parametrize("B,heads,T", [(4, 12, 197), (2, 12, 257), (3, 3, 33)])
def test_consistent_with_cvcl_attention(dev, B, heads, T):
    """probs @ v per head against cvcl_attention's output on the same fp32 qkv; float64 P V is the reference of the tau rule."""
    H = _H()
    hd, scale = 64, 0.125
    qkv = _qkv(B, heads, T, hd, torch.float32, seed=T)
    v64 = qkv.double().reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)[2]
    v32 = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)[2]
    ref64 = VC.softmax_probs(qkv.double(), B, T, heads, hd, scale) @ v64
    ref32 = VC.softmax_probs(qkv, B, T, heads, hd, scale) @ v32
    tau = VC.tau(ref32, ref64)
    qd = qkv.to(dev)
    probs = _launch(qd, B, T, heads, hd, scale, T)
    out = torch.empty(B * T, heads * hd, dtype=torch.float32, device=dev)
    H.check(H.lib().cvcl_attention(H.F32, H.ptr(qd), None, H.ptr(out), B, T, heads, hd, scale, H.stream_ptr()), "cvcl_attention")
    pv = probs.double().cpu() @ v64                                                        # [B, heads, T, hd]
    att = out.double().cpu().reshape(B, T, heads, hd).permute(0, 2, 1, 3)
    e_pv, e_att, e_pair = (float((a - b).abs().max()) for a, b in ((pv, ref64), (att, ref64), (pv, att)))
    rowsum = float((probs.double().sum(-1) - 1).abs().max())
    print(f"[probs @ v] B {B} heads {heads} T {T}: tau {tau:.3e}; probs @ v vs float64 {e_pv:.3e}, cvcl_attention vs float64 {e_att:.3e}, "
          f"probs @ v vs cvcl_attention {e_pair:.3e}; row sums off 1 by {rowsum:.3e}")
    assert e_pair <= tau and e_pv <= tau
    assert rowsum <= T * 2.0 ** -23


def test_deterministic_and_canary(dev):
    """Two launches are bit-identical; nothing is written beyond [B][heads][q_rows][T] (odd T: rows are only 4-byte aligned)."""
    H = _H()
    B, heads, T, hd = 2, 12, 197, 64
    qd = _qkv(B, heads, T, hd, torch.bfloat16, seed=3).to(dev)
    for q_rows in (1, 7, T):
        n = B * heads * q_rows * T
        buf = torch.full((n + 1024,), -7.0, dtype=torch.float32, device=dev)
        H.check(H.lib().cvcl_attention_probs(H.BF16, H.ptr(qd), H.ptr(buf), B, T, heads, hd, 0.125, q_rows, H.stream_ptr()), "probs")
        assert bool((buf[n:] == -7.0).all()) and bool((buf[:n] >= 0).all())
        again = _launch(qd, B, T, heads, hd, 0.125, q_rows)
        assert torch.equal(again.reshape(-1), buf[:n])


# ---- the model's methods ---------------------------------------------------------------------------------------------------

def _tiny_vit(dev):
    from multimodal import vision_transformer_dino_mugs as vits
    g = load_golden("vit_tiny")
    m = vits.VisionTransformer(img_size=[32], patch_size=8, embed_dim=32, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w.")})
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(dev).eval()


def test_golden_native_and_resampled_resolution(dev):
    """fp32 methods on the vit_tiny weights against the reference's own outputs, at the ViT forward's golden bound."""
    g, gt, gi = load_golden("vit_attention"), load_golden("vit_tiny"), load_golden("vit_tiny_interp")
    m = _tiny_vit(dev)
    for tag, x in (("", gt["x"]), ("_a", gi["x_a"]), ("_b", gi["x_b"])):
        attn = m.get_last_selfattention(x.to(dev))
        layers = m.get_intermediate_layers(x.to(dev), 2)
        e_a = maxrel(attn, g["attn" + tag])
        e_l = max(maxrel(a, b) for a, b in zip(layers, g["layers" + tag]))
        print(f"[golden{tag or '_native'}] attention rel err {e_a:.2e}, layers {e_l:.2e}")
        assert attn.shape == g["attn" + tag].shape and len(layers) == 2
        assert e_a < 2e-5 and e_l < 2e-5
        assert torch.equal(m.get_intermediate_layers(x.to(dev), 1)[0], layers[-1])


@functools.lru_cache(maxsize=None)
def _base(patch):
    """ViT-B/patch with the formula weights of the vit_b16 / vit_b14 goldens, a batch of 4 at 224 x 224, and the CPU restatement in
    float64, fp32 and under autocast(bfloat16)."""
    import gen_golden as G
    from multimodal import vision_transformer_dino_mugs as vits
    m = vits.vit_base(patch_size=patch, num_classes=0)
    sd = G.vit_formula_state(m.state_dict())
    assert sorted(sd.keys()) == [str(k) for k in load_golden(f"vit_b{patch}")["keys"]]
    m.load_state_dict(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        a64, l64 = VC.maps_and_layers(VC.to_dtype(sd, torch.float64), x.double(), patch, 12, 4)
        a32, l32 = VC.maps_and_layers(sd, x, patch, 12, 4)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            a16, _ = VC.maps_and_layers(sd, x, patch, 12, 1)
    return m, x, (a64, l64), (a32, l32), a16.float()


@pytest.mark.parametrize("patch", [16, 14])
def test_full_size_fp32_vs_float64(dev, patch):
    m, x, (a64, l64), (a32, l32), _ = _base(patch)
    m = m.to(dev).eval()
    m.compute_dtype = torch.float32
    xd = x.to(dev)
    attn = m.get_last_selfattention(xd)
    layers = m.get_intermediate_layers(xd, 4)
    tau_a = VC.tau(a32, a64)
    e_a = float((attn.double().cpu() - a64).abs().max())
    print(f"[ViT-B/{patch} fp32] maps {tuple(attn.shape)}: tau {tau_a:.3e}, error {e_a:.3e}")
    res = []
    for i, (got, w32, w64) in enumerate(zip(layers, l32, l64)):
        tau_l, e_l = VC.tau(w32, w64), float((got.double().cpu() - w64).abs().max())
        print(f"[ViT-B/{patch} fp32] layer {8 + i}: tau {tau_l:.3e}, error {e_l:.3e}")
        res.append((e_l, tau_l))
    assert len(layers) == 4 and layers[0].shape == l64[0].shape
    assert e_a <= tau_a
    for e_l, tau_l in res:
        assert e_l <= tau_l
    # the CLS rows of the last layer are forward()'s output: the same kernels see the same rows
    cls = m(xd)
    same = torch.equal(layers[-1][:, 0], cls)
    print(f"[ViT-B/{patch} fp32] get_intermediate_layers(x, 1)[0][:, 0] vs forward(x): bit-equal {same}, rel {maxrel(layers[-1][:, 0], cls):.2e}")
    assert maxrel(m.get_intermediate_layers(xd, 1)[0][:, 0], cls) <= 1e-6


@pytest.mark.parametrize("patch", [16, 14])
def test_bf16_maps_vs_own_fp32(dev, patch):
    m, x, _, (a32, _), a16 = _base(patch)
    m = m.to(dev).eval()
    xd = x.to(dev)
    m.compute_dtype = torch.float32
    want = m.get_last_selfattention(xd)
    m.compute_dtype = torch.bfloat16
    try:
        got = m.get_last_selfattention(xd)
    finally:
        m.compute_dtype = torch.float32
    yard = float((a16.double() - a32.double()).abs().max())
    err = float((got.double() - want.double()).abs().max())
    print(f"[ViT-B/{patch} bf16] maps vs own fp32: {err:.3e}; torch autocast(bf16) vs its fp32: {yard:.3e} -> bound {2 * yard:.3e}")
    assert got.dtype == torch.float32 and err <= 2 * yard


def test_vit_cls_attention(dev):
    from multimodal import attention_maps as A
    m, x, *_ = _base(16)
    m = m.to(dev).eval()
    for dt in (torch.float32, torch.bfloat16):
        m.compute_dtype = dt
        try:
            xd = x[:2].to(dev)
            full = m.get_last_selfattention(xd)                                            # [2, 12, 197, 197]
            per_head = A.vit_cls_attention(m, xd, heads=None)
            assert per_head.shape == (2, 12, 14, 14) and per_head.dtype == torch.float32
            assert torch.equal(per_head, full[:, :, 0, 1:].reshape(2, 12, 14, 14))         # bit for bit
            mean = A.vit_cls_attention(m, xd)
            assert mean.shape == (2, 14, 14)
            e = maxrel(mean, per_head.double().mean(1))
            print(f"[vit_cls_attention {dt}] head mean vs float64 mean: rel {e:.2e}")
            assert e <= 1e-6
            for maps in (mean, per_head):
                big = A.vit_cls_attention(m, xd, size=(224, 224), heads="mean" if maps is mean else None)
                assert big.shape == (*maps.shape[:-2], 224, 224) and torch.equal(big, A.bicubic_resize(maps, (224, 224)))
        finally:
            m.compute_dtype = torch.float32
    # a VisionEncoder wrapper is accepted as well
    enc = torch.nn.Module()
    enc.model = m
    assert torch.equal(A.vit_cls_attention(enc, x[:1].to(dev)), A.vit_cls_attention(m, x[:1].to(dev)))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_frozen_forward_untouched(dev, dt):
    """forward(x) before and after a get_last_selfattention call on the same model is bit-equal: fp32, and bf16 with the trunk
    stream enabled (two trunk streams, the benchmark's configuration)."""
    m, x, *_ = _base(16)
    m = m.to(dev).eval()
    xd = x.to(dev)
    m.compute_dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    try:
        if dt == "bf16":
            m.enable_trunk_stream(dev, n_streams=2)
        before = m(xd).clone()
        attn = m.get_last_selfattention(xd)
        layers = m.get_intermediate_layers(xd, 2)
        after = m(xd).clone()
        again = m(xd).clone()
        torch.cuda.synchronize()
        assert torch.equal(before, after) and torch.equal(before, again)
        assert attn.shape == (4, 12, 197, 197) and len(layers) == 2
    finally:
        m.enable_trunk_stream(dev, inputs=None)
        m.compute_dtype = torch.float32


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_intermediate_layers_are_the_plain_forward(dev, dt):
    """The analysis walk and the forward's plain route (fp32; bf16 with ln_fold False) are one launch sequence, vit_hip._Trunk: the
    CLS rows of the last layer are forward(x) bit for bit, and so is the last of two layers the only one of one.  No tolerance."""
    from multimodal import vision_transformer_dino_mugs as vits
    torch.manual_seed(11)
    m = vits.VisionTransformer(img_size=[224], patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    for p in m.parameters():
        p.requires_grad_(False)
        p.add_(0.05 * torch.randn_like(p))                  # biases and LayerNorm parameters off their initial 0 / 1
    m = m.to(dev).eval()
    m.compute_dtype, m.ln_fold = dt, False
    xd = torch.randn(2, 3, 224, 224).to(dev)
    last = m.get_intermediate_layers(xd, 1)[0]
    assert last.shape == (2, 197, 128) and last.dtype == torch.float32
    assert torch.equal(last[:, 0], m(xd))
    assert torch.equal(m.get_intermediate_layers(xd, 2)[-1], last)


def _patched_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return lambda name, pretrained: vits.VisionTransformer(img_size=[224], patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4,
                                                           qkv_bias=True, num_classes=0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_self_attention_maps_and_eval_entry(dev, tmp_path, monkeypatch):
    """MultiModalLitModel.self_attention_maps returns forward()'s logits bit for bit and the head-mean CLS maps; eval.py
    --attention_maps on a synthetic ViT checkpoint writes cams.npy [trials, 4, gh, gw] (text: the trial's map repeated), the
    prediction records are those of a run without the flag, --plot_attention writes its overlays; attention_maps keeps raising."""
    import eval as ev
    import train
    import multimodal.multimodal as mm
    from multimodal import attention_maps as A
    from multimodal.multimodal_data_module import SyntheticEvalTrials
    from multimodal.multimodal_lit import MultiModalLitModel
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mm, "load_model", _patched_vit())
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --vit_dino "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features "
            f"--checkpoint_callback True --logger False --exp_name {exp}").split()
    with contextlib.redirect_stdout(io.StringIO()):
        train.main(argv)
        lit = MultiModalLitModel.load_from_checkpoint(ev.resolve_checkpoint(exp), map_location=dev).to(dev).eval()
    trials = SyntheticEvalTrials(6, 2350, seed=0 + 4, eval_type="image")
    imgs, label, n, _ = trials[0]
    imgs, tok, ln = imgs.to(dev), label.view(1, -1).to(dev), torch.tensor([n], device=dev)
    with torch.no_grad():
        lpi, lpt = lit(imgs, tok, ln)
        lpi2, lpt2, maps = lit.self_attention_maps(imgs, tok, ln)
        assert torch.equal(lpi, lpi2) and torch.equal(lpt, lpt2)
        assert maps.shape == (4, 14, 14) and torch.equal(maps, A.vit_cls_attention(lit.vision_encoder, imgs))
        with pytest.raises(NotImplementedError, match="ResNeXt encoder only"):
            lit.attention_maps(imgs, tok, ln)
    for eval_type in ("image", "text"):
        base = ["--checkpoint", exp, "--eval_dataset", "synthetic", "--eval_type", eval_type, "--n_trials", "6", "--trial_batch", "4"]
        with contextlib.redirect_stdout(io.StringIO()):
            plain = ev.main(ev._parser().parse_args(base))
            d = tmp_path / f"maps_{eval_type}"
            mapped = ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d)] + (["--plot_attention"] if eval_type == "image" else [])))
        assert json.dumps(plain) == json.dumps(mapped)
        cams = np.load(d / "cams.npy")
        assert cams.shape == (6, 4, 14, 14) and cams.dtype == np.float32
        trials = SyntheticEvalTrials(6, 2350, seed=0 + 4, eval_type=eval_type)
        if eval_type == "image":
            assert len(list(d.glob("*_attn_map.png"))) == 6
            for i in range(6):
                want = A.vit_cls_attention(lit.vision_encoder, trials[i][0].to(dev))
                assert maxrel(torch.from_numpy(cams[i]), want) <= 1e-5, i       # (other batch size: the GEMMs may tile differently)
        else:
            for i in range(6):
                img = trials[i][0]
                want = A.vit_cls_attention(lit.vision_encoder, img.reshape(1, *img.shape[-3:]).to(dev))
                assert maxrel(torch.from_numpy(cams[i]), want.expand(4, -1, -1)) <= 1e-5, i
                assert all(np.array_equal(cams[i, 0], cams[i, j]) for j in range(1, 4))
