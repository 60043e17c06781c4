"""Grad-CAM on the MI355X (csrc/gradcam.hip, multimodal/attention_maps.py) against the reference's arithmetic on the CPU in float64:
torch autograd through fc -> (F.normalize) -> <out, target> and F.interpolate(bicubic, align_corners=False), starting from the
device's own layer-4 map, fc output and fc weights -- so the tests pin the Grad-CAM, not the (separately tested) trunk."""
import argparse
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 1e-5


def _encoder(dtype, E=64, embedding_type="flat", seed=0):
    from multimodal.multimodal import VisionEncoder
    args = argparse.Namespace(embedding_type=embedding_type, embedding_dim=E, pretrained_cnn=False, cnn_model="resnext50_32x4d",
                              cnn_dino=False, vit_dino=False, finetune_cnn=False)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(args)
    ve.to("cuda:0").eval()
    ve.set_compute_dtype(dtype)
    return ve


def _images(n, seed=1, size=224):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, size, size, generator=g).to("cuda:0")


def _forward(resnet, x):
    from multimodal.attention_maps import Hook
    with torch.no_grad(), Hook(resnet.layer4, requires_grad=False) as hook:
        f = resnet(x)
        A = hook.activation
    return f, A


def _err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def _ref_grad_f(f, T, normalize):
    """d<out, t>/df in float64 through torch autograd: f [N, E], T [M, E] -> [M, N, E] (every target for every image)."""
    M = T.shape[0]
    fr = f.detach().double().cpu()[None].expand(M, -1, -1).clone().requires_grad_(True)
    out = F.normalize(fr, p=2, dim=-1) if normalize else fr
    out.backward(T.detach().double().cpu()[:, None, :].expand_as(out))
    return fr.grad


def _ref_cams(A, f, W, T, normalize, pair_index=None, grad_to_bf16=False):
    """CPU float64 Grad-CAM of image n for target m: the gradient at the map is (d<out,t>/df W) / hw at every position (fc of the
    avgpool); alpha = its spatial mean; cam = relu(sum_c alpha_c A_c).  -> [N, M, h, w] (or the pairs of pair_index [(n, m)])."""
    A64 = A.detach().double().cpu()
    N, C, h, w = A64.shape
    W64 = W.detach().double().cpu()
    out = []
    for m0 in range(0, T.shape[0], 128):
        g = _ref_grad_f(f, T[m0:m0 + 128], normalize)                 # [m, N, E]
        grad = (g @ W64) / (h * w)                                     # [m, N, C]: the map's gradient at every position
        if grad_to_bf16:
            grad = grad.float().bfloat16().double()                    # autograd stores the map's gradient in the map's dtype
        grad_map = grad[..., None, None].expand(-1, -1, -1, h, w)
        alpha = grad_map.mean((3, 4))
        out.append(torch.einsum("mnc,nchw->nmhw", alpha, A64).clamp(min=0))
    cams = torch.cat(out, 1)
    if pair_index is not None:
        return torch.stack([cams[n, m] for n, m in pair_index])
    return cams


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("normalize", [False, True])
def test_gradcam_matches_cpu_autograd(dtype, normalize):
    from multimodal import ops
    from multimodal.attention_maps import Hook, gradCAM
    ve = _encoder(dtype)
    model = ve.model
    x = _images(8)
    f, A = _forward(model, x)
    T = torch.randn(8, f.shape[1], generator=torch.Generator().manual_seed(2)).to("cuda:0")

    # the bridge: with a gradient-requiring hook the output is bit-identical, and the map's gradient is d_pooled / hw at every
    # position, in the map's dtype and layout
    before = {n: p.requires_grad for n, p in model.named_parameters()}
    for p in model.parameters():
        p.requires_grad_(False)
    try:
        with Hook(model.layer4) as hook:
            out = model(x)
            assert torch.equal(out.detach(), f)
            (ops.l2_normalize(out) if normalize else out).backward(T)
            g = hook.gradient
    finally:
        for n, p in model.named_parameters():
            p.requires_grad_(before[n])
    assert g is not None and g.dtype == dtype and g.shape == A.shape and g.stride() == A.stride()
    gf = torch.stack([_ref_grad_f(f[i:i + 1], T[i:i + 1], normalize)[0, 0] for i in range(8)])     # d<out_i, t_i>/df_i
    want_g = ((gf @ model.fc.weight.detach().double().cpu()) / 49)[..., None, None].expand(-1, -1, 7, 7)
    if dtype == torch.float32:
        assert _err(g, want_g) <= BOUND
        grad = want_g
    else:
        # autograd's rounding to bf16: equal to the float64 value rounded, up to a rounding tie moved by the fp32 arithmetic before it
        rounded = want_g.float().bfloat16().double()
        diff = (g.double().cpu() - rounded).abs()
        assert float((diff / rounded.abs().clamp_min(1e-30)).max()) <= 2.0 ** -7
        assert float((diff > 0).double().mean()) < 1e-3
        grad = g.double().cpu()                   # the CPU computation below runs on the same bf16 gradient and the same bf16 map
    want = (grad.mean((2, 3), keepdim=True) * A.double().cpu()).sum(1).clamp(min=0)
    assert want.max() > 0

    cam = gradCAM(model, x, T, model.layer4, normalize_features=normalize, resize=False)
    assert {n: p.requires_grad for n, p in model.named_parameters()} == before
    assert cam.shape == (8, 1, 7, 7) and cam.dtype == torch.float32
    assert _err(cam[:, 0], want) <= BOUND
    big = gradCAM(model, x, T, model.layer4, normalize_features=normalize)
    assert big.shape == (8, 1, 224, 224)
    want_big = F.interpolate(want[:, None], (224, 224), mode="bicubic", align_corners=False)
    assert _err(big, want_big) <= BOUND


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gradcam_pairs_all_layouts(dtype):
    from multimodal.attention_maps import gradCAM, gradCAM_pairs
    ve = _encoder(dtype)
    model = ve.model
    N = 16
    x = _images(N, seed=3)
    f, A = _forward(model, x)
    E = f.shape[1]
    gen = torch.Generator().manual_seed(4)
    for normalize in (False, True):
        T = torch.randn(40, E, generator=gen).to("cuda:0")
        got = gradCAM_pairs(ve, x, T, normalize, pairs="all")
        assert got.shape == (N, 40, 7, 7)
        want = _ref_cams(A, f, model.fc.weight, T, normalize)
        assert _err(got, want) <= BOUND
        up = gradCAM_pairs(ve, x, T, normalize, pairs="all", resize=(33, 17))
        assert up.shape == (N, 40, 33, 17)
        assert _err(up, F.interpolate(want.reshape(N * 40, 1, 7, 7), (33, 17), mode="bicubic", align_corners=False).view(N, 40, 33, 17)) <= BOUND

        Td = torch.randn(N, E, generator=gen).to("cuda:0")
        diag = gradCAM_pairs(ve, x, Td, normalize, pairs="diagonal", resize=True)
        assert diag.shape == (N, 224, 224)
        d7 = gradCAM_pairs(ve, x, Td, normalize, pairs="diagonal")
        want_d = _ref_cams(A, f, model.fc.weight, Td, normalize, [(i, i) for i in range(N)])
        assert _err(d7, want_d) <= BOUND
        # the reference-style call on the same batch: exact in fp32; in bf16 its map gradient is rounded to bf16 first (autograd)
        ref = gradCAM(model, x, Td, model.layer4, normalize_features=normalize, resize=True)[:, 0]
        assert _err(diag, ref) <= (BOUND if dtype == torch.float32 else 1e-2)

        Ti = torch.randn(N * 4, E, generator=gen).to("cuda:0")           # image n with targets 4n .. 4n + 3
        bi = gradCAM_pairs(ve, x, Ti, normalize, pairs=("block", 4, "image"))
        assert bi.shape == (N, 4, 7, 7)
        want_i = _ref_cams(A, f, model.fc.weight, Ti, normalize, [(n, 4 * n + j) for n in range(N) for j in range(4)])
        assert _err(bi.reshape(-1, 7, 7), want_i) <= BOUND

        Tt = torch.randn(N // 4, E, generator=gen).to("cuda:0")          # target j with images 4j .. 4j + 3
        bt = gradCAM_pairs(ve, x, Tt, normalize, pairs=("block", 4, "text"))
        assert bt.shape == (N // 4, 4, 7, 7)
        want_t = _ref_cams(A, f, model.fc.weight, Tt, normalize, [(4 * j + i, j) for j in range(N // 4) for i in range(4)])
        assert _err(bt.reshape(-1, 7, 7), want_t) <= BOUND


def test_gradcam_pairs_full_vocabulary():
    """All pairs against M = 2350 targets (the vocabulary size): every target tile, including the ragged last one."""
    from multimodal.attention_maps import gradCAM_pairs
    ve = _encoder(torch.bfloat16)
    x = _images(4, seed=5)
    f, A = _forward(ve.model, x)
    T = torch.randn(2350, f.shape[1], generator=torch.Generator().manual_seed(6)).to("cuda:0")
    got = gradCAM_pairs(ve, x, T, True, pairs="all")
    assert got.shape == (4, 2350, 7, 7)
    assert _err(got, _ref_cams(A, f, ve.model.fc.weight, T, True)) <= BOUND


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gradcam_pairs_near_cancellation(dtype):
    """Targets t = n^ + delta z with the terms of R - s U each ~5x the result (delta picked on the CPU for that cancellation).  The
    device's exact-fp32 contraction holds the bound; the same arithmetic with P = T W and Q = n^ W rounded to bf16 (a plain bf16
    contraction) visibly does not."""
    from multimodal.attention_maps import gradCAM_pairs
    ve = _encoder(dtype)
    x = _images(8, seed=7)
    f, A = _forward(ve.model, x)
    W64 = ve.model.fc.weight.detach().double().cpu()
    A64, f64 = A.double().cpu(), f.double().cpu()
    nhat = F.normalize(f64, dim=1)
    z = torch.randn(f64.shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    z = z / z.norm(dim=1, keepdim=True)
    U = torch.einsum("nc,nchw->nhw", nhat @ W64, A64)
    scale = (f64.norm(dim=1) * 49)[:, None, None]

    def terms(T64, Pq=lambda v: v):
        s = (nhat * T64).sum(1)[:, None, None]
        R = torch.einsum("nc,nchw->nhw", Pq(T64 @ W64), A64)
        Ub = torch.einsum("nc,nchw->nhw", Pq(nhat @ W64), A64)
        return (s * U).abs().max() / scale.max(), ((R - s * Ub) / scale).clamp(min=0)

    def cancellation(delta):
        big, cam = terms(nhat + delta * z)
        return float(big / cam.max())
    deltas = [0.05 * 1.5 ** i for i in range(40)]
    delta = min(deltas, key=lambda d: abs(cancellation(d) - 5.0))
    assert 3.0 < cancellation(delta) < 8.0
    T64 = nhat + delta * z
    want = _ref_cams(A, f, ve.model.fc.weight, T64.float(), True, [(i, i) for i in range(8)])
    got = gradCAM_pairs(ve, x, T64.float().cuda(), True, pairs="diagonal")
    assert _err(got, want) <= BOUND
    _, bf = terms(T64.float().double(), lambda v: v.float().bfloat16().double())
    assert _err(bf, want) > 10 * BOUND


def test_bicubic_resize_matches_interpolate():
    from multimodal.attention_maps import bicubic_resize
    g = torch.Generator().manual_seed(9)
    for (h, w), (Hh, Ww) in (((7, 7), (224, 224)), ((5, 9), (33, 17)), ((40, 30), (13, 11)), ((7, 7), (7, 7)), ((3, 6), (224, 230))):
        x = torch.randn(6, h, w, generator=g)
        want = F.interpolate(x[:, None], (Hh, Ww), mode="bicubic", align_corners=False)[:, 0]     # torch's fp32 arithmetic, as called
        got = bicubic_resize(x.to("cuda:0"), (Hh, Ww))
        assert got.shape == (6, Hh, Ww)
        assert _err(got, want) <= 2e-6, ((h, w), (Hh, Ww))


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_act_grad_generic_layouts(act_dtype, grad_dtype):
    from multimodal.attention_maps import gradCAM_with_act_and_grad
    g = torch.Generator().manual_seed(10)
    for (N, C, h, w) in ((3, 256, 14, 14), (2, 2048, 7, 7), (2, 64, 5, 3)):
        act = torch.randn(N, C, h, w, generator=g).relu().to(act_dtype)
        grad = torch.randn(N, C, h, w, generator=g).to(grad_dtype)
        a64, g64 = act.double(), grad.double()
        want = (a64 * g64.mean((2, 3), keepdim=True)).sum(1, keepdim=True).clamp(min=0)
        nchw = gradCAM_with_act_and_grad(act.cuda(), grad.cuda())
        nhwc = gradCAM_with_act_and_grad(act.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2),
                                         grad.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2))
        mixed = gradCAM_with_act_and_grad(act.cuda(), grad.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2))
        for got in (nchw, nhwc, mixed):
            assert got.shape == (N, 1, h, w)
            assert _err(got, want) <= BOUND


def test_unsupported_encoders_and_cpu_tensors():
    from multimodal import _hip as H
    from multimodal import vision_transformer_dino_mugs as vits
    from multimodal.attention_maps import gradCAM_pairs
    import multimodal.multimodal as mm
    x = _images(2)
    T = torch.randn(2, 64).cuda()
    spatial = _encoder(torch.float32, embedding_type="spatial")
    with pytest.raises(NotImplementedError, match="spatial"):
        gradCAM_pairs(spatial, x, T)
    with pytest.raises(NotImplementedError, match="spatial"):
        gradCAM_pairs(spatial.model, x, T)
    args = argparse.Namespace(embedding_type="flat", embedding_dim=64, pretrained_cnn=False, cnn_dino=False, vit_dino=True,
                              finetune_cnn=False)
    orig = mm.load_model
    mm.load_model = lambda name, pretrained: vits.vit_small(patch_size=16, num_classes=0)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            vit = mm.VisionEncoder(args)
    finally:
        mm.load_model = orig
    with pytest.raises(NotImplementedError, match="ViT"):
        gradCAM_pairs(vit, x, T)
    flat = _encoder(torch.float32)
    with pytest.raises(H.CvclError):
        gradCAM_pairs(flat, x.cpu(), T.cpu())
    with pytest.raises(ValueError):
        gradCAM_pairs(flat, x, torch.randn(3, 64).cuda(), pairs="diagonal")


def test_eval_entry_attention_maps(dev, tmp_path, monkeypatch):
    """eval.py --attention_maps: cams.npy [n_trials, 4, 7, 7] from the same pass as the logits equals per-trial gradCAM calls, and the
    predictions are those of a run without the flag, for both evaluation types; --plot_attention writes one PNG per trial."""
    import json
    import numpy as np
    import eval as ev
    import train
    from multimodal.attention_maps import gradCAM
    from multimodal.multimodal_data_module import SyntheticEvalTrials
    from multimodal.multimodal_lit import MultiModalLitModel
    monkeypatch.chdir(tmp_path)
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features "
            f"--checkpoint_callback True --logger False --exp_name {exp}").split()
    with contextlib.redirect_stdout(io.StringIO()):
        train.main(argv)
    lit = MultiModalLitModel.load_from_checkpoint(ev.resolve_checkpoint(exp), map_location=dev).to(dev).eval()
    for eval_type in ("image", "text"):
        base = ["--checkpoint", exp, "--eval_dataset", "synthetic", "--eval_type", eval_type, "--n_trials", "6", "--trial_batch", "4"]
        with contextlib.redirect_stdout(io.StringIO()):
            plain = ev.main(ev._parser().parse_args(base))
            d = tmp_path / f"maps_{eval_type}"
            mapped = ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d)] + (["--plot_attention"] if eval_type == "image" else [])))
        assert json.dumps(plain) == json.dumps(mapped)
        cams = np.load(d / "cams.npy")
        assert cams.shape == (6, 4, 7, 7) and cams.dtype == np.float32
        if eval_type == "image":
            assert len(list(d.glob("*_attn_map.png"))) == 6
        trials = SyntheticEvalTrials(6, 2350, seed=0 + 4, eval_type=eval_type)
        resnet = lit.vision_encoder.model
        for i in range(6):
            if eval_type == "image":                      # the trial's 4 images w.r.t. its label
                imgs, label, n, _ = trials[i]
                with torch.no_grad():
                    t = lit.encode_text(label.view(1, -1).to(dev), torch.tensor([n], device=dev))
                imgs, t = imgs.to(dev), t.expand(4, -1).contiguous()
            else:                                         # the trial's image w.r.t. its 4 labels
                img, labels, lens, _ = trials[i]
                with torch.no_grad():
                    t = lit.encode_text(labels.to(dev), torch.as_tensor(lens, device=dev).long())
                imgs = img.reshape(1, *img.shape[-3:]).expand(4, -1, -1, -1).contiguous().to(dev)
            want = gradCAM(resnet, imgs, t, resnet.layer4, normalize_features=True, resize=False)[:, 0]
            # two fp32 evaluations of the same maps (closed-form contraction vs backward + act/grad), each ~1e-5 from float64
            assert _err(torch.from_numpy(cams[i]), want) <= 5 * BOUND, (eval_type, i)
