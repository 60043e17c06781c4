"""Per-word Grad-CAM of the captioning LM on the MI355X (csrc/lstm.hip, csrc/head.hip, multimodal/attention_maps.py): against the reference's
own maps (tests/golden/caption_gradcam.npz), against the per-word loop through the autograd bridges on the device, against float64
autograd on the CPU at configuration size, the seed kernel alone against cvcl_lstm_cell_bwd on replicated rows, and the interface.

Bound (caption_gradcam_common.bound): max|got - want| / max|want| <= min(2e-4, max(1e-5, 10 ref32_dev)), ref32_dev the distance of
the reference arithmetic's own fp32 run from its float64 run (stored in the fixture; computed on the CPU for the other cases).

Measured on one MI355X (max|got - want| / max|want|; every bound came out as 1.0e-05, one as 1.1e-05):
  fixture            plain 7.8e-07, normalized 2.9e-07 (the reference's own fp32 run: 6.6e-07, 2.9e-07)
  loop, fp32 trunk   plain 1.9e-06 / normalized 1.7e-06 vs float64, 1.4e-06 / 1.5e-06 vs the loop
  loop, bf16 trunk   plain 1.8e-06 / normalized 2.3e-06 vs float64 from the bf16 map, 1.4e-03 / 5.0e-03 vs the loop (allowed 1e-2)
  config size        targets 1.8e-06 / 2.0e-06, maps 2.5e-06 / 2.2e-06
  batch of one vs the same caption in a batch of four: 2.3e-06"""
import contextlib
import io

import pytest
import torch

import caption_gradcam_common as K
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _nhwc(A):
    return A.to(DEV).contiguous(memory_format=torch.channels_last)


# ---- 1. the reference's own maps -----------------------------------------------------------------------------------------------

def test_reference_fixture():
    from multimodal.attention_maps import caption_gradcam_from_features
    fx = load_golden("caption_gradcam")
    lm, w = K.toy_language_model(DEV)
    A = fx["map"]
    f = (A.double().mean(dim=(2, 3)) @ w["fc.weight"].double().t() + w["fc.bias"].double()).float()
    y, n = fx["y"].to(DEV), fx["y_len"].to(DEV)
    # the contraction takes C % 32 == 0 (the trunk's 2048): the fixture's 48 channels are followed by 16 zero channels with zero
    # fc columns, which add exact zeros to every sum; f above comes from the 48 real ones
    pad = (-K.C) % 32
    A_dev = _nhwc(torch.cat([A, A.new_zeros(K.B, pad, K.HW, K.HW)], 1))
    W_dev = torch.cat([w["fc.weight"], torch.zeros(K.E, pad)], 1).to(DEV)
    for case in fx["cases"]:
        got = caption_gradcam_from_features(A_dev, f.to(DEV), W_dev, lm, y, n, normalize_features=case == "normalized")
        want = fx[f"{case}.cam64"]
        assert got.shape == want.shape and got.dtype == torch.float32
        e, bnd = K.err(got, want), K.bound(fx[f"{case}.ref32_dev"])
        print(f"fixture {case}: {e:.2e} (bound {bnd:.1e}, ref32_dev {float(fx[f'{case}.ref32_dev']):.2e})")
        assert e <= bnd
        for b in range(K.B):
            assert bool((got[b, int(n[b]) - 1:] == 0).all())


# ---- 2. the per-word loop on the device ----------------------------------------------------------------------------------------

def _lit(dtype, normalize, E=128, seed=0):
    from multimodal.multimodal import TextEncoder, VisionEncoder
    from multimodal.multimodal_data_module import read_vocab
    from multimodal.multimodal_lit import MultiModalLitModel
    args = K.lm_args(E, normalize)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(args)
        lit = MultiModalLitModel(ve, TextEncoder(read_vocab(), 2048, args), args)
    lit.to(DEV).eval()
    ve.set_compute_dtype(dtype)
    return lit


def _captions(B, L, V, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(4, V, (B, L), generator=g)
    n = torch.randint(3, L + 1, (B,), generator=g) if lens is None else torch.as_tensor(lens)
    n[0] = L
    y[:, 0] = 2
    for b in range(B):
        y[b, int(n[b]) - 1] = 3
        y[b, int(n[b]):] = 0
    return y, n


def _loop_port(lit, x, y, n):
    """The reference's procedure on the device: hook layer4 with a gradient, token-wise loss, one backward per word, the map from
    the hooked activation and minus its gradient.  (One trunk pass for the batch: the loss of caption b reaches image b only.)"""
    from multimodal.attention_maps import Hook, gradCAM_with_act_and_grad
    resnet = lit.vision_encoder.model
    saved = {k: p.requires_grad for k, p in lit.named_parameters()}
    for p in lit.parameters():
        p.requires_grad_(False)
    B, L = y.shape
    cams = torch.zeros(B, L - 1, 7, 7, device=DEV)
    try:
        with Hook(resnet.layer4) as hook, torch.enable_grad():
            loss = lit.calculate_ce_loss(y, n, x=x, tokenwise=True)[0]
            for b in range(B):
                for p in range(int(n[b]) - 1):
                    hook.data.grad = None
                    loss[b, p].backward(retain_graph=True)
                    cams[b, p] = gradCAM_with_act_and_grad(hook.activation.detach(), -hook.gradient)[b, 0]
            A = hook.activation.detach()
    finally:
        for k, p in lit.named_parameters():
            p.requires_grad_(saved[k])
    return cams, A


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("normalize", [False, True])
def test_equals_per_word_loop(dtype, normalize):
    from multimodal.attention_maps import Hook, gradCAM_captions
    lit = _lit(dtype, normalize)
    resnet = lit.vision_encoder.model
    B, L = 8, 12
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    y, n = _captions(B, L, lit.language_model.text_encoder.vocab_size, seed=2)
    y, n = y.to(DEV), n.to(DEV)
    got = gradCAM_captions(lit, x, y, n)
    assert got.shape == (B, L - 1, 7, 7)
    loop, A = _loop_port(lit, x, y, n)
    assert A.dtype == dtype
    with torch.no_grad(), Hook(resnet.layer4, requires_grad=False):
        f = resnet(x)
    _g, want, dev32, _ = K.reference(A, f, resnet.fc.weight, K.weights_of(lit.language_model), y, normalize)
    bnd = K.bound(dev32)
    e64, eloop = K.err(got, want), K.err(got, loop)
    print(f"loop {dtype} normalize={normalize}: vs float64 {e64:.2e}, vs loop {eloop:.2e}, loop vs float64 {K.err(loop, want):.2e} "
          f"(bound {bnd:.1e}, ref32_dev {dev32:.2e})")
    assert float(want.max()) > 0
    # float64 on the CPU from the device's own map (bf16 trunk: the bf16 map as stored), fc output and weights
    assert e64 <= bnd
    if dtype == torch.float32:
        assert eloop <= bnd
    else:
        # the loop's gradient at the map is stored by autograd in the map's dtype: alpha is rounded to bf16 (2^-9 relative per
        # channel) before the contraction, the batched path keeps it in fp32.  That rounding, and only that, is allowed here -- the
        # bound test_gradcam_gpu.py uses for the same comparison.
        assert eloop <= 1e-2
    for b in range(B):
        assert bool((got[b, int(n[b]) - 1:] == 0).all())


# ---- 3. configuration size against float64 -------------------------------------------------------------------------------------

def test_config_size_vs_float64():
    from multimodal.attention_maps import Hook, caption_gradcam_from_features, caption_seed_targets
    lit = _lit(torch.float32, False, E=512, seed=3)
    resnet, lm = lit.vision_encoder.model, lit.language_model
    B, L = 256, 25
    V = lm.text_encoder.vocab_size
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
    y, n = _captions(B, L, V, seed=6)
    n[1] = 3                                                                     # the shortest possible caption: <sos> w <eos>
    y[1, 2], y[1, 3:] = 3, 0
    with torch.no_grad(), Hook(resnet.layer4, requires_grad=False) as hook:
        f = resnet(x)
        A = hook.activation
    assert A.shape == (B, 2048, 7, 7) and f.shape == (B, 512)
    sample = sorted({0, 1, int(n.argmax()), int(n.argmin())} | set(range(2, B, 17)))
    assert len(sample) >= 16 and int(n[sample].max()) == L and int(n[sample].min()) == 3
    yd, nd = y.to(DEV), n.to(DEV)
    w = K.weights_of(lm)
    for normalize in (False, True):
        targets = caption_seed_targets(f, lm, yd, nd, normalize).view(B, L - 1, -1)
        cams = caption_gradcam_from_features(A, f, resnet.fc.weight, lm, yd, nd, normalize_features=normalize)
        assert cams.shape == (B, L - 1, 7, 7)
        g64, cam64, dev_cam, dev_g = K.reference(A[sample], f[sample], resnet.fc.weight, w, y[sample], normalize)
        eg, ec = K.err(-targets[sample], g64), K.err(cams[sample], cam64)
        print(f"config size normalize={normalize}: targets {eg:.2e} (bound {K.bound(dev_g):.1e}, ref32_dev {dev_g:.2e}), "
              f"maps {ec:.2e} (bound {K.bound(dev_cam):.1e}, ref32_dev {dev_cam:.2e})")
        assert float(cam64.max()) > 0
        assert eg <= K.bound(dev_g)
        assert ec <= K.bound(dev_cam)
        for b in sample:
            assert bool((cams[b, int(n[b]) - 1:] == 0).all()) and bool((targets[b, int(n[b]) - 1:] == 0).all())


# ---- 4. the seed kernel alone --------------------------------------------------------------------------------------------------

def _cell_inputs(B, L, Hd, lens, seed):
    g = torch.Generator().manual_seed(seed)
    gact = torch.rand(B * L, 4 * Hd, generator=g)
    gact[:, 2 * Hd:3 * Hd] = gact[:, 2 * Hd:3 * Hd] * 2 - 1                        # the cell gate is a tanh
    csave = torch.randn(B * L, Hd, generator=g)
    c0 = torch.randn(B, Hd, generator=g)
    d_out = torch.randn(B * L, Hd, generator=g)
    return gact.to(DEV), csave.to(DEV), c0.to(DEV), d_out.to(DEV), torch.as_tensor(lens, dtype=torch.int64).to(DEV)


# Hd 36: rows Hd / 4 = 135 work items, one partial 256-thread block; Hd 260: 975 items, three full blocks and a tail of 207
@pytest.mark.parametrize("Hd", [36, 260])
@pytest.mark.parametrize("s,with_c0,inject", [(2, False, True), (2, False, False), (0, True, True), (0, False, True), (0, True, False)])
def test_seed_kernel_equals_cell_bwd_on_replicated_rows(s, with_c0, inject, Hd):
    from multimodal import _hip as H
    B, L = 5, 7
    lens = [7, 2, 5, 0, 3]                                                          # captions 1 and 3 have ended at s = 2, 3 even at s = 0
    n_act = 3
    rows = B * n_act
    gact, csave, c0, d_out, ln = _cell_inputs(B, L, Hd, lens, seed=10 + s)
    g = torch.Generator().manual_seed(99)
    dh = torch.randn(rows, Hd, generator=g).to(DEV)
    dc = torch.randn(rows, Hd, generator=g).to(DEV)
    lib, st = H.lib(), H.stream_ptr()

    # the existing entries on explicitly replicated captions: row r is caption r % B
    rep = torch.arange(rows, device=DEV) % B
    gact_r = gact.view(B, L, -1)[rep].reshape(rows * L, -1).contiguous()
    csave_r = csave.view(B, L, -1)[rep].reshape(rows * L, -1).contiguous()
    ln_r = ln[rep].contiguous()
    dh_r, dc_r = dh.clone(), dc.clone()
    if inject:                                                                      # what cvcl_lstm_add_dout leaves on zeros
        dh_r[:B] = torch.where((ln > s)[:, None], d_out.view(B, L, Hd)[:, s], torch.zeros((), device=DEV))
        dc_r[:B] = 0
    dG_r = torch.full((rows * L, 4 * Hd), float("nan"), device=DEV)
    carry_r = torch.full((rows, Hd), float("nan"), device=DEV)
    if with_c0:
        H.check(lib.cvcl_lstm_cell_bwd_first(H.ptr(gact_r), H.ptr(csave_r), H.ptr(c0[rep].contiguous()), H.ptr(ln_r), H.ptr(dh_r),
                                             H.ptr(dc_r), H.ptr(dG_r), H.ptr(carry_r), rows, L, Hd, st), "cvcl_lstm_cell_bwd_first")
    else:
        H.check(lib.cvcl_lstm_cell_bwd(H.ptr(gact_r), H.ptr(csave_r), H.ptr(ln_r), s, H.ptr(dh_r), H.ptr(dc_r), H.ptr(dG_r),
                                       H.ptr(carry_r), rows, L, Hd, st), "cvcl_lstm_cell_bwd")
    want_dG = dG_r.view(rows, L, 4 * Hd)[:, s]

    dh_s, dc_s = dh.clone(), dc.clone()
    if inject:                                                                      # the joining block's dh / dc must not be read
        dh_s[:B] = float("nan")
        dc_s[:B] = float("nan")
    dG = torch.full((rows, 4 * Hd), float("nan"), device=DEV)
    carry = torch.full((rows, Hd), float("nan"), device=DEV)
    H.check(lib.cvcl_lstm_cell_bwd_seeds(H.ptr(gact), H.ptr(csave), H.ptr(c0) if with_c0 else None, H.ptr(ln), s,
                                         H.ptr(d_out) if inject else None, H.ptr(dh_s), H.ptr(dc_s), H.ptr(dG), H.ptr(carry), B, L, Hd,
                                         rows, st), "cvcl_lstm_cell_bwd_seeds")
    torch.cuda.synchronize()
    assert not torch.isnan(dG).any() and not torch.isnan(carry).any() and not torch.isnan(dc_s).any()
    assert torch.equal(dG, want_dG)
    assert torch.equal(carry, carry_r)
    assert torch.equal(dc_s, dc_r)
    masked = (ln <= s)[rep]
    assert bool(masked.any()) and bool((dG[masked] == 0).all()) and bool((dG[~masked] != 0).any())
    if not inject:
        assert torch.equal(dh_s, dh)                                                # dh itself is read-only


def test_l2norm_seeds_equals_l2norm_bwd_per_block():
    from multimodal import _hip as H
    B, Kk, E = 7, 5, 96
    g = torch.Generator().manual_seed(3)
    f = torch.randn(B, E, generator=g).to(DEV)
    f[2] = 0                                                                        # norm below eps: the clamp branch
    dy = torch.randn(Kk * B, E, generator=g).to(DEV)
    lib, st = H.lib(), H.stream_ptr()
    yv, norm = torch.empty_like(f), torch.empty(B, device=DEV)
    H.check(lib.cvcl_l2norm_fwd(H.ptr(f), H.ptr(yv), H.ptr(norm), B, E, 1e-12, st), "cvcl_l2norm_fwd")
    want = torch.empty(Kk, B, E, device=DEV)
    for p in range(Kk):
        H.check(lib.cvcl_l2norm_bwd(H.ptr(yv), H.ptr(norm), dy.data_ptr() + p * B * E * 4, want.data_ptr() + p * B * E * 4, B, E, 1e-12, st),
                "cvcl_l2norm_bwd")
    got = torch.empty(B * Kk, E, device=DEV)
    H.check(lib.cvcl_l2norm_bwd_seeds(H.ptr(yv), H.ptr(norm), H.ptr(dy), H.ptr(got), B, Kk, E, 1e-12, st), "cvcl_l2norm_bwd_seeds")
    assert torch.equal(got.view(B, Kk, E), want.permute(1, 0, 2))
    H.check(lib.cvcl_l2norm_bwd_seeds(None, None, H.ptr(dy), H.ptr(got), B, Kk, E, 1e-12, st), "cvcl_l2norm_bwd_seeds")
    assert torch.equal(got.view(B, Kk, E), dy.view(Kk, B, E).permute(1, 0, 2))


# ---- 5. the interface ----------------------------------------------------------------------------------------------------------

def test_interface_and_model_state():
    import numpy as np
    from analysis_tools.multimodal_visualization import gradCAM_for_captioning_lm
    from multimodal.attention_maps import Hook, bicubic_resize, gradCAM_captions
    lit = _lit(torch.float32, True, E=64, seed=4)
    lit.train()                                                                     # the flags must survive, whatever they are
    lit.vision_encoder.model.fc.weight.requires_grad_(False)
    B, L = 4, 10
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(7)).to(DEV)
    y, n = _captions(B, L, lit.language_model.text_encoder.vocab_size, seed=8, lens=[10, 6, 3, 8])
    yd, nd = y.to(DEV), n.to(DEV)
    flags = {k: m.training for k, m in lit.named_modules()}
    req = {k: p.requires_grad for k, p in lit.named_parameters()}
    before = {k: v.detach().clone() for k, v in lit.state_dict().items()}

    cams = gradCAM_captions(lit, x, yd, nd)
    assert cams.shape == (B, L - 1, 7, 7) and cams.dtype == torch.float32 and not cams.requires_grad
    assert torch.equal(gradCAM_captions(lit, x, yd, nd), cams)                     # a second call: bit-identical
    big = gradCAM_captions(lit, x, yd, nd, resize=True)
    assert big.shape == (B, L - 1, 224, 224) and torch.equal(big, bicubic_resize(cams, (224, 224)))

    b, nb = 1, 6
    one = gradCAM_captions(lit, x[b:b + 1], yd[b:b + 1, :nb].contiguous(), nd[b:b + 1])
    ret = gradCAM_for_captioning_lm(lit, x[b].cpu(), y[b, :nb], n[b])              # host inputs, as the reference's callers pass them
    assert isinstance(ret, list) and len(ret) == nb and ret[0] is None
    for step in range(1, nb):
        assert isinstance(ret[step], np.ndarray) and ret[step].shape == (7, 7) and ret[step].dtype == np.float32
        assert np.array_equal(ret[step], one[0, step - 1].cpu().numpy())           # a batch-of-one call, bit for bit
    sub = gradCAM_for_captioning_lm(lit, x[b], yd[b, :nb], nd[b], steps=[3, 0, 5])
    assert sub[1] is None and np.array_equal(sub[0], ret[3]) and np.array_equal(sub[2], ret[5])
    # row b of the larger batch: the same maps up to the summation order of GEMMs (and trunk passes) with another M -- within the
    # bound of 1, its ref32_dev from the reference arithmetic on the CPU (fp32 vs float64) on this caption, starting from the
    # device's own map and fc output of the batch-of-one trunk pass (eval mode, as gradCAM_captions runs it)
    resnet = lit.vision_encoder.model
    lit.eval()
    with torch.no_grad(), Hook(resnet.layer4, requires_grad=False) as hook:
        f1 = resnet(x[b:b + 1])
        A1 = hook.activation
    lit.train()
    _g, want1, dev32, _ = K.reference(A1, f1, resnet.fc.weight, K.weights_of(lit.language_model), y[b:b + 1, :nb], True)
    bnd = K.bound(dev32)
    e, e1, eb = K.err(one[0], cams[b, :nb - 1]), K.err(one[0], want1[0]), K.err(cams[b, :nb - 1], want1[0])
    print(f"batch of one vs row {b} of a batch of {B}: {e:.2e}; vs float64 {e1:.2e} / {eb:.2e} (bound {bnd:.1e}, ref32_dev {dev32:.2e})")
    assert e <= bnd and e1 <= bnd and eb <= bnd and bool((cams[b, nb - 1:] == 0).all())

    assert {k: m.training for k, m in lit.named_modules()} == flags
    assert {k: p.requires_grad for k, p in lit.named_parameters()} == req
    assert all(p.grad is None for p in lit.parameters())
    after = lit.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())               # BatchNorm buffers included
