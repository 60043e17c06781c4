"""GPU parity: backward of the ResNeXt trunk (--finetune_cnn) vs the oracle's autograd.

Each operator of multimodal/trunk_train.py is checked against torch-CPU autograd of the same op (fp32 mode tight;
bf16 mode against fp32 maths of bf16-rounded operands, loose), then the whole trunk's parameter gradients against
the oracle's functional ResNeXt (fp32 parity mode)."""
import pytest
import torch
import torch.nn.functional as F

import cvcl_oracle as O
from conftest import maxrel

pytestmark = pytest.mark.gpu


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _cdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def _tol(dt, f32, bf16):
    return bf16 if dt == "bf16" else f32


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,k_keep", [(1000, 64, 256, 256), (5000, 128, 64, 64), (77, 256, 512, 512), (20000, 64, 160, 147),
                                          (300000, 128, 256, 256), (4096, 1024, 512, 512)])
def test_gemm_tn_exact_on_small_integers(dev, dt, M, N, K, k_keep):
    """Weight-gradient GEMM C = A^T B (contraction over rows, split + fixed-order reduction): with small-integer operands
    every product and partial sum is exact in fp32, so the result must equal the float64 reference bit for bit --
    this pins the ds_read_b64_tr_b16 fragment layout (any row/column mix-up changes the answer) and the split logic."""
    from multimodal.trunk_train import _gemm_tn
    g = torch.Generator().manual_seed(M + N)
    a = torch.randint(-3, 4, (M, N), generator=g).float()
    b = torch.randint(-3, 4, (M, K), generator=g).float()
    ref = (a.double().t() @ b.double())[:, :k_keep].float()
    ad, bd = a.to(_cdt(dt)).to(dev), b.to(_cdt(dt)).to(dev)
    out = _gemm_tn(ad, bd, k_keep)
    out2 = _gemm_tn(ad, bd, k_keep)
    assert out.shape == (N, k_keep) and torch.equal(out.cpu(), ref) and torch.equal(out, out2)


@pytest.mark.parametrize("B,S,C_,stride", [(2, 8, 128, 1), (2, 16, 256, 2), (3, 14, 1024, 2), (4, 28, 512, 1), (3, 56, 128, 1), (2, 56, 256, 2),
                                           (5, 7, 1024, 1)])
def test_gconv_wgrad_exact_on_small_integers(dev, B, S, C_, stride):
    """bf16 grouped-conv weight gradient is exact on small integers: the one-pass band kernel (ring of input rows; bands pipelined through
    registers at 56 / 28 / 14 / 7 pixels with stride 1, staged in place for the 56-pixel stride-2 layer; several bands and images per
    workgroup) on the trunk's own feature-map sizes."""
    from multimodal import _hip as H
    g = torch.Generator().manual_seed(C_ + S)
    cg = C_ // 32
    x = torch.randint(-2, 3, (B, C_, S, S), generator=g).float().requires_grad_(False)
    w = torch.zeros(C_, cg, 3, 3, requires_grad=True)
    y = F.conv2d(x.double(), w.double(), None, stride, 1, 1, 32)
    dy = torch.randint(-2, 3, y.shape, generator=g).float()
    (gw,) = torch.autograd.grad(y, w, dy.double())
    xd, dyd = nhwc(x).bfloat16().to(dev), nhwc(dy).bfloat16().to(dev)
    dw = torch.empty(C_, cg, 3, 3, device=dev)
    nb = H.lib().cvcl_gconv3x3_wgrad_workspace_bytes(B, S, S, C_, stride)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    H.check(H.lib().cvcl_gconv3x3_wgrad(H.ptr(xd), H.ptr(dyd), H.ptr(dw), B, S, S, C_, 32, stride, H.ptr(ws), nb, H.stream_ptr()), "wgrad")
    assert torch.equal(dw.cpu(), gw.float())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,S,K,N,stride", [(2, 8, 64, 128, 1), (3, 7, 256, 64, 1), (2, 8, 256, 512, 2), (1, 14, 1024, 2048, 2)])
def test_conv1x1_grads(dev, dt, B, S, K, N, stride):
    from multimodal.trunk_train import Conv1x1
    g = torch.Generator().manual_seed(K + N)
    q = O.bf16_round if dt == "bf16" else (lambda t: t)
    x = q(torch.randn(B, K, S, S, generator=g)).requires_grad_()
    w = (torch.randn(N, K, 1, 1, generator=g) / K ** 0.5).requires_grad_()
    y = F.conv2d(x, q(w), None, stride)
    dy = q(torch.randn(y.shape, generator=g))
    y.backward(dy)
    xd = nhwc(x.detach()).to(_cdt(dt)).to(dev).requires_grad_()
    wd = w.detach().to(dev).requires_grad_()
    yd, st = Conv1x1.apply(xd, wd, stride)
    assert maxrel(st.double().sum(0)[0].float(), yd.detach().float().reshape(-1, N).sum(0)) < (2e-2 if dt == 'bf16' else 1e-4)
    dyd = nhwc(dy).to(_cdt(dt)).to(dev)
    yd.backward(dyd)
    assert maxrel(yd.float(), nhwc(y.detach())) < _tol(dt, 2e-5, 8e-3)
    assert maxrel(xd.grad.float(), nhwc(x.grad)) < _tol(dt, 2e-5, 8e-3)
    assert wd.grad.dtype == torch.float32 and maxrel(wd.grad, w.grad) < _tol(dt, 5e-5, 8e-3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,S,C_,stride", [(2, 8, 128, 1), (2, 16, 256, 2), (1, 14, 512, 1), (3, 14, 1024, 2), (2, 7, 1024, 1)])
def test_gconv_grads(dev, dt, B, S, C_, stride):
    from multimodal.trunk_train import GroupedConv3x3
    g = torch.Generator().manual_seed(C_ + S)
    q = O.bf16_round if dt == "bf16" else (lambda t: t)
    cg = C_ // 32
    x = q(torch.randn(B, C_, S, S, generator=g)).requires_grad_()
    w = (torch.randn(C_, cg, 3, 3, generator=g) / (3 * cg ** 0.5)).requires_grad_()
    y = F.conv2d(x, q(w), None, stride, 1, 1, 32)
    dy = q(torch.randn(y.shape, generator=g))
    y.backward(dy)
    xd = nhwc(x.detach()).to(_cdt(dt)).to(dev).requires_grad_()
    wd = w.detach().to(dev).requires_grad_()
    yd, _st = GroupedConv3x3.apply(xd, wd, stride)
    dyd = nhwc(dy).to(_cdt(dt)).to(dev)
    yd.backward(dyd)
    assert maxrel(yd.float(), nhwc(y.detach())) < _tol(dt, 2e-5, 8e-3)
    assert maxrel(xd.grad.float(), nhwc(x.grad)) < _tol(dt, 2e-5, 8e-3)
    assert maxrel(wd.grad, w.grad) < _tol(dt, 5e-5, 8e-3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stem_maxpool_avgpool_addrelu_grads(dev, dt):
    from multimodal.trunk_train import AddRelu, AvgPool, MaxPool3x3s2, StemConv
    g = torch.Generator().manual_seed(5)
    q = O.bf16_round if dt == "bf16" else (lambda t: t)
    x = torch.randn(2, 3, 32, 32, generator=g)
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).requires_grad_()
    y = F.conv2d(q(x), q(w), None, 2, 3)
    dy = q(torch.randn(y.shape, generator=g))
    y.backward(dy)
    xd, wd = x.to(dev), w.detach().to(dev).requires_grad_()
    yd, _st = StemConv.apply(xd, wd, _cdt(dt))
    dyd = nhwc(dy).to(_cdt(dt)).to(dev)
    yd.backward(dyd)
    assert maxrel(yd.float(), nhwc(y.detach())) < _tol(dt, 2e-5, 8e-3)
    assert maxrel(wd.grad, w.grad) < _tol(dt, 5e-5, 8e-3)
    # max pool (ties exist after bf16 rounding: first arg-max wins, like torch's CPU kernel)
    a = q(torch.randn(2, 64, 16, 16, generator=g)).requires_grad_()
    p = F.max_pool2d(a, 3, 2, 1)
    dp = q(torch.randn(p.shape, generator=g))
    p.backward(dp)
    ad = nhwc(a.detach()).to(_cdt(dt)).to(dev).requires_grad_()
    pd = MaxPool3x3s2.apply(ad)
    dpd = nhwc(dp).to(_cdt(dt)).to(dev)
    pd.backward(dpd)
    assert torch.equal(pd.float().cpu(), nhwc(p.detach())) and maxrel(ad.grad.float(), nhwc(a.grad)) < _tol(dt, 1e-6, 8e-3)
    # relu(a + b), avg pool
    u, v = q(torch.randn(2, 64, 4, 4, generator=g)).requires_grad_(), q(torch.randn(2, 64, 4, 4, generator=g)).requires_grad_()
    o = torch.relu(u + v).mean(dim=(2, 3))
    do = torch.randn(o.shape, generator=g)
    o.backward(do)
    ud, vd = (nhwc(t.detach()).to(_cdt(dt)).to(dev).requires_grad_() for t in (u, v))
    od = AvgPool.apply(AddRelu.apply(ud, vd))
    dod = do.to(dev)
    od.backward(dod)
    assert maxrel(od, o.detach()) < _tol(dt, 1e-6, 8e-3)
    assert maxrel(ud.grad.float(), nhwc(u.grad)) < _tol(dt, 1e-6, 8e-3) and torch.equal(ud.grad, vd.grad)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows_shape,C_", [((2, 9, 9), 64), ((3, 28, 28), 256), ((4, 2, 2), 2048)])
def test_batchnorm_train_grads(dev, dt, relu, rows_shape, C_):
    from multimodal.trunk_train import BatchNormTrain
    g = torch.Generator().manual_seed(C_)
    q = O.bf16_round if dt == "bf16" else (lambda t: t)
    B, Hh, Ww = rows_shape
    x = q(torch.randn(B, C_, Hh, Ww, generator=g) * 1.5 + 0.3).requires_grad_()
    gamma = (torch.rand(C_, generator=g) + 0.5).requires_grad_()
    beta = (torch.randn(C_, generator=g) * 0.3).requires_grad_()
    rm, rv = torch.randn(C_, generator=g) * 0.1, torch.rand(C_, generator=g) + 0.5
    rm_o, rv_o = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm_o, rv_o, gamma, beta, True, 0.1, 1e-5)
    if relu:
        y = torch.relu(y)
    dy = q(torch.randn(y.shape, generator=g))
    y.backward(dy)
    xd = nhwc(x.detach()).to(_cdt(dt)).to(dev).requires_grad_()
    gd, bd = gamma.detach().to(dev).requires_grad_(), beta.detach().to(dev).requires_grad_()
    rmd, rvd, nbt = rm.to(dev), rv.to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    yd = BatchNormTrain.apply(xd, None, gd, bd, rmd, rvd, nbt, relu)
    dyd = nhwc(dy).to(_cdt(dt)).to(dev)
    yd.backward(dyd)
    assert maxrel(yd.float(), nhwc(y.detach())) < _tol(dt, 2e-5, 1e-2)
    assert maxrel(rmd, rm_o) < 1e-5 and maxrel(rvd, rv_o) < 1e-5 and int(nbt) == 1
    if dt == "f32":          # in bf16 the ReLU mask comes from the rounded y: compare only where unambiguous
        assert maxrel(xd.grad, nhwc(x.grad)) < 2e-4
        assert maxrel(gd.grad, gamma.grad) < 1e-4 and maxrel(bd.grad, beta.grad) < 1e-4
    else:
        assert maxrel(gd.grad, gamma.grad) < 3e-2 and maxrel(bd.grad, beta.grad) < 3e-2
        assert maxrel(xd.grad.float(), nhwc(x.grad)) < 5e-2


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("rows_shape,C_", [((2, 9, 9), 256), ((3, 14, 14), 1024), ((5, 2, 2), 2048)])
def test_bn_add_relu_tail_grads(dev, dt, rows_shape, C_):
    """Fused Bottleneck tail out = relu(bn3(raw) + identity): output and the gradients of raw, identity, gamma, beta."""
    from multimodal.trunk_train import BnAddRelu
    g = torch.Generator().manual_seed(C_ + 1)
    q = O.bf16_round if dt == "bf16" else (lambda t: t)
    B, Hh, Ww = rows_shape
    x = q(torch.randn(B, C_, Hh, Ww, generator=g) * 1.5 + 0.3).requires_grad_()
    idn = q(torch.randn(B, C_, Hh, Ww, generator=g)).requires_grad_()
    gamma = (torch.rand(C_, generator=g) + 0.5).requires_grad_()
    beta = (torch.randn(C_, generator=g) * 0.3).requires_grad_()
    rm, rv = torch.zeros(C_), torch.ones(C_)
    y = torch.relu(F.batch_norm(x, rm.clone(), rv.clone(), gamma, beta, True, 0.1, 1e-5) + idn)
    dy = q(torch.randn(y.shape, generator=g))
    y.backward(dy)
    xd, idd = (nhwc(t.detach()).to(_cdt(dt)).to(dev).requires_grad_() for t in (x, idn))
    gd, bd = gamma.detach().to(dev).requires_grad_(), beta.detach().to(dev).requires_grad_()
    rmd, rvd, nbt = rm.to(dev), rv.to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    yd = BnAddRelu.apply(xd, None, gd, bd, rmd, rvd, nbt, idd)
    dyd = nhwc(dy).to(_cdt(dt)).to(dev)
    yd.backward(dyd)
    assert maxrel(yd.float(), nhwc(y.detach())) < _tol(dt, 2e-5, 1e-2)
    if dt == "f32":
        assert maxrel(xd.grad, nhwc(x.grad)) < 2e-4 and maxrel(idd.grad, nhwc(idn.grad)) < 1e-6
        assert maxrel(gd.grad, gamma.grad) < 1e-4 and maxrel(bd.grad, beta.grad) < 1e-4
    else:
        assert maxrel(gd.grad, gamma.grad) < 3e-2 and maxrel(bd.grad, beta.grad) < 3e-2
        assert maxrel(xd.grad.float(), nhwc(x.grad)) < 5e-2


def _randomised_params(seed):
    p = O.resnext50_random_params(seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in list(p.keys()):
        if ("bn" in k or "downsample.1" in k) and k.endswith(".weight"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
    return p


@pytest.mark.parametrize("B,S", [(4, 64), (2, 96)])
def test_trunk_parameter_grads_vs_oracle_fp32(dev, B, S):
    """Whole differentiable trunk (fp32 parity mode, train-mode BN): pooled features, running statistics and the
    gradient of every one of the 159 trunk parameters for a random upstream gradient, vs oracle autograd."""
    from multimodal.resnext import ResNet
    p = _randomised_params(3)
    g = torch.Generator().manual_seed(B + S)
    x = torch.randn(B, 3, S, S, generator=g)
    names = [k for k in p if p[k].dtype.is_floating_point and "running" not in k and not k.startswith("fc.")]
    po = {k: (v.clone().requires_grad_() if k in names else v.clone()) for k, v in p.items()}
    stats_o = {}
    pooled_o, _ = O.resnext50_forward(po, x, True, None, stats_out=stats_o)
    dp = torch.randn(pooled_o.shape, generator=g)
    pooled_o.backward(dp)
    model = ResNet()
    sd = model.state_dict()
    for k, v in p.items():
        sd[k].copy_(v)
    model = model.to(dev).train()
    pooled, fmap = model.trunk(x.to(dev))
    assert pooled.requires_grad and fmap.shape == (B, 2048, S // 32, S // 32)
    dpd = dp.to(dev)
    pooled.backward(dpd)
    assert maxrel(pooled.detach(), pooled_o.detach()) < 2e-4
    got = dict(model.named_parameters())
    # Parameter gradients of a train-mode-BN ResNeXt over a handful of samples are ill-conditioned even in fp32: the
    # oracle's own gradients move by up to 0.27 max-rel (cosine >= 0.9995) when its input is scaled by (1 + 1e-7),
    # because ReLU / max-pool decisions flip (measured in the build container).  Element-exactness is carried by the
    # per-operator tests above; here every parameter's gradient must agree in direction and norm.
    worst_cos, worst_l2 = ("", 1.0), ("", 0.0)
    for k in names:
        assert got[k].grad is not None and got[k].grad.dtype == torch.float32, k
        a, b = got[k].grad.cpu().flatten().double(), po[k].grad.flatten().double()
        cos = float(F.cosine_similarity(a, b, dim=0))
        l2 = float((a - b).norm() / b.norm())
        if cos < worst_cos[1]:
            worst_cos = (k, cos)
        if l2 > worst_l2[1]:
            worst_l2 = (k, l2)
    print(f"trunk grads B={B} S={S}: min cosine {worst_cos[1]:.6f} at {worst_cos[0]}, max rel-L2 {worst_l2[1]:.2e} at {worst_l2[0]}")
    assert len(names) == 159 and worst_cos[1] > 0.998 and worst_l2[1] < 0.06, (worst_cos, worst_l2)
    for k in ("bn1.running_mean", "layer4.2.bn3.running_var"):
        assert maxrel(model.state_dict()[k], stats_o[k]) < 1e-4


def test_trunk_bf16_grads_finite_deterministic(dev):
    """bf16 fine-tuning step: gradients are finite and bit-reproducible, and the last block's BN gradients point the
    same way as in fp32 mode.  Nothing stronger is meaningful end to end: on a random-init ResNeXt the ORACLE's own
    gradients with bf16-rounded forward activations (exact fp32 backward) have a median cosine of 0.22 to its fp32
    gradients (max 0.96 at layer4.2.bn3.bias; measured in the build container, B=8 64x64), i.e. the map
    activations -> parameter gradients is chaotic.  Exactness of the bf16 kernels is carried by the per-operator tests."""
    from multimodal.resnext import ResNet
    torch.manual_seed(0)
    model = ResNet().to(dev).train()
    x = torch.randn(16, 3, 128, 128, device=dev)
    dp = torch.randn(16, 2048, device=dev)
    grads = {}
    for cdt in (torch.float32, torch.bfloat16, torch.bfloat16):
        model.compute_dtype = cdt
        model.zero_grad(set_to_none=True)
        model.recalibrate_centres()                               # ... and the same (zero) storage centres: they track step by step
        with torch.no_grad():                                     # same running statistics going in every time
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.reset_running_stats()
        pooled, _ = model.trunk(x)
        pooled.backward(dp)
        cur = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
        assert len(cur) == 159 and all(torch.isfinite(v).all() for v in cur.values())
        if cdt == torch.bfloat16 and "bf" in grads:
            assert all(torch.equal(cur[k], grads["bf"][k]) for k in cur)          # deterministic (no atomics anywhere)
        grads["bf" if cdt == torch.bfloat16 else "f32"] = cur
    for k in ("layer4.2.bn3.bias", "layer4.2.bn3.weight"):
        a, b = grads["f32"][k].flatten().double(), grads["bf"][k].flatten().double()
        cos = float(F.cosine_similarity(a, b, dim=0))
        print(k, "cos", round(cos, 4))
        assert cos > 0.8, (k, cos)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_weight_gradient_stream_is_bit_identical(dev, monkeypatch, cdt):
    """trunk_train runs the weight-gradient kernels on their own HIP stream and stores them into param.grad when the backward
    pass ends ($CVCL_WGRAD_STREAM, default on): same gradients, bit for bit, as the one-stream form where autograd accumulates
    them -- including accumulation over two backward passes -- and torch.autograd.grad on the Functions themselves still works."""
    from multimodal.resnext import ResNet
    from multimodal import trunk_train as TT
    torch.manual_seed(1)
    model = ResNet().to(dev).train()
    model.compute_dtype = cdt
    x = torch.randn(6, 3, 96, 96, device=dev)
    dp = torch.randn(6, 2048, device=dev)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CVCL_WGRAD_STREAM", mode)
        model.zero_grad(set_to_none=True)
        model.recalibrate_centres()                                   # both modes start from the same (zero) storage centres
        for _ in range(2):                                        # the second pass accumulates into existing .grad tensors
            with torch.no_grad():
                for m in model.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.reset_running_stats()
            pooled, _ = model.trunk(x)
            pooled.backward(dp)
        torch.cuda.synchronize()
        assert not TT._WGRAD_PENDING
        res[mode] = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    assert len(res["0"]) == len(res["1"]) == 159
    for k, v in res["0"].items():
        assert v.shape == dict(model.named_parameters())[k].shape and torch.equal(v, res["1"][k]), k
    # the Functions called directly (no deferral requested) still return the weight gradient through autograd
    w = torch.nn.Parameter(torch.randn(64, 128, 1, 1, device=dev))
    xx = torch.randn(2, 8, 8, 128, device=dev).to(cdt)
    y, _ = TT.Conv1x1.apply(xx, w, 1)
    (gw,) = torch.autograd.grad(y, w, torch.ones_like(y))
    assert gw.shape == w.shape and torch.isfinite(gw).all()


def test_trunk_train_refuses_sizes_that_are_no_multiple_of_32(dev):
    """A 200 x 200 batch would reach layer3.0 as a 25 x 25 map, whose stride-2 backward reads the zero-stuffed gradient (always
    [B, 2 Ho, 2 Wo, C]) at the wrong pitch: the fine-tuning trunk refuses it like the frozen one does, before any kernel runs --
    no BatchNorm buffer has moved."""
    from multimodal import _hip as H
    from multimodal.resnext import ResNet
    model = ResNet().to(dev).train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for shape in ((2, 3, 200, 200), (2, 3, 224, 200), (2, 3, 200, 224)):
        with pytest.raises(H.CvclError, match="multiples of 32"):
            model.trunk(torch.zeros(shape, device=dev))
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


@pytest.mark.parametrize("op", ["gconv", "conv1x1"])
def test_stride2_backward_refuses_an_odd_map(dev, op):
    """the two stride-2 backward passes themselves refuse an odd saved map (forward is fine: 25 -> 13) before they launch anything"""
    from multimodal import _hip as H
    from multimodal.trunk_train import Conv1x1, GroupedConv3x3
    x = torch.ones(2, 25, 25, 128, dtype=torch.bfloat16, device=dev).requires_grad_()
    if op == "gconv":
        w = torch.ones(128, 4, 3, 3, device=dev).requires_grad_()
        y, _st = GroupedConv3x3.apply(x, w, 2)
    else:
        w = torch.ones(256, 128, 1, 1, device=dev).requires_grad_()
        y, _st = Conv1x1.apply(x, w, 2)
    assert y.shape[1:3] == (13, 13)
    with pytest.raises(H.CvclError, match="even map"):
        y.backward(torch.ones_like(y))
    assert x.grad is None and w.grad is None


def test_finetune_cnn_training_step(dev):
    """reference config with --finetune_cnn (multimodal.py:175-179): the trunk's parameters receive gradients and an
    AdamW step changes them; the default (frozen) configuration leaves them untouched."""
    import contextlib
    import io
    import train
    argv = ("--dataset synthetic --batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --lambda_lm 0 "
            "--optimize_unused --finetune_cnn --fast_dev_run --checkpoint_callback False --logger False").split()
    with contextlib.redirect_stdout(io.StringIO()):
        trainer, lit = train.main(argv)
    w = lit.vision_encoder.model.layer1[0].conv2.weight
    assert w.requires_grad and w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().sum()) > 0
