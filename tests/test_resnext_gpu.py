"""GPU parity: ResNeXt-50 trunk kernels through the C ABI vs the oracle.

fp32 mode (parity mode) is compared with the oracle's fp32 arithmetic; bf16 mode with the oracle's
storage-point emulation (``quant=bf16_round``: operands/stored activations rounded to bf16, fp32
accumulation and statistics), which isolates kernel bugs from expected bf16 rounding.
The oracle's ResNeXt is parity-unpinned by the reference (torchvision absent): see oracle header."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cvcl_oracle as O
from conftest import maxrel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    return _hip


def _t(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def _q(dt):
    return O.bf16_round if dt == "bf16" else (lambda t: t)


def nhwc(t):          # NCHW (oracle) -> NHWC contiguous
    return t.permute(0, 2, 3, 1).contiguous()


def pack(H, dt, kind, w, dev):
    cd = H.BF16 if dt == "bf16" else H.F32
    cout, cing, k, _ = w.shape
    nb = H.lib().cvcl_packed_weight_bytes(cd, kind, cout, cing, k)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    wd = w.to(dev).contiguous()
    H.check(H.lib().cvcl_pack_conv_weight(cd, kind, H.ptr(wd), H.ptr(buf), cout, cing, k, H.stream_ptr()), "pack")
    torch.cuda.synchronize()
    return buf


def stats_tensor(rows, C, dev):
    return torch.full((rows, 2, C), float("nan"), device=dev)


def check_stats(stats, rows, y):
    s = stats[:rows].double().sum(dim=0).cpu()
    yd = y.double().cpu().reshape(-1, y.shape[-1])
    assert maxrel(s[0], yd.sum(dim=0)) < 2e-5
    assert maxrel(s[1], (yd * yd).sum(dim=0)) < 2e-5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("B,S", [(2, 64), (1, 224)])
def test_stem(H, dev, dt, B, S, centred):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, 3, S, S, generator=g) + (1.5 if centred else 0.0)      # (a DC component: channel means far from zero)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    q = _q(dt)
    ref = F.conv2d(q(x), q(w), None, 2, 3)
    cen = ref.mean(dim=(0, 2, 3)) + 0.01 * torch.randn(64, generator=g) if centred else None   # centred storage: round(y - c)
    if centred:
        ref = ref - cen[None, :, None, None]
    cend = cen.to(dev) if centred else None
    cd = H.BF16 if dt == "bf16" else H.F32
    wp = pack(H, dt, H.PACK_STEM7, w, dev)
    y = torch.empty(B, S // 2, S // 2, 64, dtype=_t(dt), device=dev)
    rows = H.lib().cvcl_stem_conv_stats_rows(cd, B, S, S)
    st = stats_tensor(rows, 64, dev)
    xd = x.to(dev)
    H.check(H.lib().cvcl_stem_conv7x7(cd, H.ptr(xd), H.ptr(wp), H.ptr(y), H.ptr(st), rows, H.ptr(cend), B, S, S, H.stream_ptr()), "stem")
    assert maxrel(y.float(), nhwc(ref)) < (6e-3 if dt == "bf16" else (1e-4 if centred else 2e-5))
    check_stats(st, rows, y)


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("B,S", [(3, 64), (2, 224), (2, 72), (1, 96), (300, 32)])
def test_fused_stem_pool_is_bit_identical_to_the_two_passes(H, dev, B, S, centred):
    """Round 5: conv1 + bn1 + relu + maxpool in one kernel (cvcl_stem_pool), its BatchNorm statistics from a statistics-only stem pass
    (cvcl_stem_conv7x7 with y = NULL) -- against the two-pass form it replaces (store the raw stem output, then cvcl_bn_relu_maxpool):
    the same statistics rows and the same pooled tensor, bit for bit (incl. odd pooled sizes: S = 72 -> 36 -> 18, 96 -> 48 -> 24,
    and more items than workgroups)."""
    g = torch.Generator().manual_seed(S + B)
    x = (torch.randn(B, 3, S, S, generator=g) + (1.5 if centred else 0.0)).to(dev)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    wp = pack(H, "bf16", H.PACK_STEM7, w, dev)
    cen = (0.3 * torch.randn(64, generator=g)).to(dev) if centred else None
    rows = H.lib().cvcl_stem_conv_stats_rows(H.BF16, B, S, S)
    raw = torch.empty(B, S // 2, S // 2, 64, dtype=torch.bfloat16, device=dev)
    st_a, st_b = stats_tensor(rows, 64, dev), stats_tensor(rows, 64, dev)
    H.check(H.lib().cvcl_stem_conv7x7(H.BF16, H.ptr(x), H.ptr(wp), H.ptr(raw), H.ptr(st_a), rows, H.ptr(cen), B, S, S, H.stream_ptr()), "stem")
    H.check(H.lib().cvcl_stem_conv7x7(H.BF16, H.ptr(x), H.ptr(wp), None, H.ptr(st_b), rows, H.ptr(cen), B, S, S, H.stream_ptr()), "stem stats only")
    assert torch.equal(st_a, st_b)
    scale = (0.5 + torch.rand(64, generator=g)).to(dev)
    shift = (0.3 * torch.randn(64, generator=g)).to(dev)
    Hp = (S // 2 - 1) // 2 + 1
    two = torch.empty(B, Hp, Hp, 64, dtype=torch.bfloat16, device=dev)
    H.check(H.lib().cvcl_bn_relu_maxpool(H.BF16, H.ptr(raw), H.ptr(scale), H.ptr(shift), H.ptr(two), B, S // 2, S // 2, 64, H.stream_ptr()), "maxpool")
    assert H.lib().cvcl_stem_pool_supported(H.BF16, S, S)
    one = torch.full((B, Hp, Hp, 64), float("nan"), dtype=torch.bfloat16, device=dev)
    H.check(H.lib().cvcl_stem_pool(H.BF16, H.ptr(x), H.ptr(wp), H.ptr(scale), H.ptr(shift), H.ptr(cen), H.ptr(one), B, S, S, H.stream_ptr()), "stem_pool")
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    assert float(two.float().abs().max()) > 0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,Hh,Ww", [(2, 16, 16), (1, 15, 17), (3, 14, 9), (1, 7, 7), (2, 113, 112), (2, 112, 112), (1, 1, 5), (1, 2, 2)])
def test_bn_relu_maxpool_shapes(H, dev, dt, B, Hh, Ww):
    """relu(bn(x)) -> max_pool2d(3, stride 2, pad 1) (torchvision ResNet stem, reference multimodal.py:155-158) on even and odd
    extents: a thread owns two output rows (round 5), the last one of an odd output height on its own; borders clamp into the
    window they belong to."""
    g = torch.Generator().manual_seed(Hh * 31 + Ww)
    Cn = 64
    x = _q(dt)(torch.randn(B, Cn, Hh, Ww, generator=g) * 2)
    scale, shift = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    ref = F.max_pool2d(torch.relu(x.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]), 3, 2, 1)
    cd = H.BF16 if dt == "bf16" else H.F32
    xd = nhwc(x).to(_t(dt)).to(dev)
    Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    y = torch.full((B, Ho, Wo, Cn), float("nan"), dtype=_t(dt), device=dev)
    sc_d, sh_d = scale.to(dev), shift.to(dev)
    H.check(H.lib().cvcl_bn_relu_maxpool(cd, H.ptr(xd), H.ptr(sc_d), H.ptr(sh_d), H.ptr(y), B, Hh, Ww, Cn, H.stream_ptr()), "maxpool")
    assert ref.shape == (B, Cn, Ho, Wo) and torch.isfinite(y.float()).all()
    assert maxrel(y.float(), nhwc(ref.float())) < (5e-3 if dt == "bf16" else 1e-6)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_finalize_and_maxpool(H, dev, dt):
    g = torch.Generator().manual_seed(2)
    B, S, Cn = 2, 16, 64
    raw = (torch.randn(B, Cn, S, S, generator=g) * 2 + 0.5)
    raw = _q(dt)(raw)
    p = {"bn.weight": torch.rand(Cn, generator=g) + 0.5, "bn.bias": torch.randn(Cn, generator=g),
         "bn.running_mean": torch.randn(Cn, generator=g), "bn.running_var": torch.rand(Cn, generator=g) + 0.5,
         "bn.num_batches_tracked": torch.tensor(3)}
    so = {}
    yo = torch.relu(O.batch_norm(raw, p, "bn", True, so))
    pool_o = F.max_pool2d(yo, 3, 2, 1)
    cd = H.BF16 if dt == "bf16" else H.F32
    xr = nhwc(raw).to(_t(dt)).to(dev)
    rows = H.lib().cvcl_col_stats_rows(B * S * S)
    st = stats_tensor(rows, Cn, dev)
    H.check(H.lib().cvcl_col_stats(cd, H.ptr(xr), B * S * S, Cn, H.ptr(st), rows, H.stream_ptr()), "col_stats")
    check_stats(st, rows, xr)
    d = {k: v.clone().to(dev) for k, v in p.items()}
    scale, shift = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    H.check(H.lib().cvcl_bn_finalize(H.ptr(st), rows, B * S * S, H.ptr(d["bn.weight"]), H.ptr(d["bn.bias"]),
                                     H.ptr(d["bn.running_mean"]), H.ptr(d["bn.running_var"]),
                                     H.ptr(d["bn.num_batches_tracked"]), 0.1, 1e-5, H.ptr(scale), H.ptr(shift), None, Cn,
                                     H.stream_ptr()), "bn_finalize")
    assert maxrel(d["bn.running_mean"], so["bn.running_mean"]) < 1e-5
    assert maxrel(d["bn.running_var"], so["bn.running_var"]) < 1e-5
    assert int(d["bn.num_batches_tracked"]) == 4
    y = torch.empty(B, S // 2, S // 2, Cn, dtype=_t(dt), device=dev)
    H.check(H.lib().cvcl_bn_relu_maxpool(cd, H.ptr(xr), H.ptr(scale), H.ptr(shift), H.ptr(y), B, S, S, Cn, H.stream_ptr()), "maxpool")
    assert maxrel(y.float(), nhwc(_q(dt)(pool_o))) < (5e-3 if dt == "bf16" else 1e-5)
    # eval-mode affine
    H.check(H.lib().cvcl_bn_eval_affine(H.ptr(d["bn.weight"]), H.ptr(d["bn.bias"]), H.ptr(d["bn.running_mean"]),
                                        H.ptr(d["bn.running_var"]), 1e-5, H.ptr(scale), H.ptr(shift), None, Cn, H.stream_ptr()), "affine")
    ref_scale = d["bn.weight"].cpu() / torch.sqrt(d["bn.running_var"].cpu() + 1e-5)
    assert maxrel(scale, ref_scale) < 1e-6
    # centred storage: the same statistics of a tensor stored as y - c give the same scale, a shift that applies to the stored
    # tensor, and running statistics of y itself (include/cvcl_hip.h "Centred storage")
    cen = (raw.mean(dim=(0, 2, 3)) + 0.05 * torch.randn(Cn, generator=g))
    xc = nhwc(_q(dt)(raw - cen[None, :, None, None])).to(_t(dt)).to(dev)
    H.check(H.lib().cvcl_col_stats(cd, H.ptr(xc), B * S * S, Cn, H.ptr(st), rows, H.stream_ptr()), "col_stats")
    d2 = {k: v.clone().to(dev) for k, v in p.items()}
    scale2, shift2, cend = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev), cen.to(dev)
    H.check(H.lib().cvcl_bn_finalize(H.ptr(st), rows, B * S * S, H.ptr(d2["bn.weight"]), H.ptr(d2["bn.bias"]),
                                     H.ptr(d2["bn.running_mean"]), H.ptr(d2["bn.running_var"]),
                                     H.ptr(d2["bn.num_batches_tracked"]), 0.1, 1e-5, H.ptr(scale2), H.ptr(shift2), H.ptr(cend), Cn,
                                     H.stream_ptr()), "bn_finalize")
    tol = 1e-2 if dt == "bf16" else 1e-4
    assert maxrel(d2["bn.running_mean"], so["bn.running_mean"]) < tol and maxrel(d2["bn.running_var"], so["bn.running_var"]) < tol
    y_c = xc.float() * scale2 + shift2                                    # the affine applies to the stored (centred) tensor
    assert maxrel(torch.relu(y_c), nhwc(yo)) < (2e-2 if dt == "bf16" else 1e-4)
    H.check(H.lib().cvcl_bn_eval_affine(H.ptr(d["bn.weight"]), H.ptr(d["bn.bias"]), H.ptr(d["bn.running_mean"]),
                                        H.ptr(d["bn.running_var"]), 1e-5, H.ptr(scale2), H.ptr(shift2), H.ptr(cend), Cn, H.stream_ptr()), "affine")
    want = d["bn.bias"].cpu() - (d["bn.running_mean"].cpu() - cen) * ref_scale
    assert maxrel(shift2, want) < 1e-5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C_,S,stride,B", [(128, 16, 1, 2), (256, 16, 2, 2), (256, 28, 1, 1), (512, 14, 2, 3),
                                           (512, 14, 1, 2), (1024, 14, 2, 2), (1024, 7, 1, 5), (128, 56, 1, 1)])
@pytest.mark.parametrize("centred", [False, True])
def test_gconv(H, dev, dt, C_, S, stride, B, centred):
    """grouped 3x3, 32 groups, all channels-per-group the network uses (4, 8, 16, 32), both strides,
    with the producer's BN+ReLU fused into the operand load and zero padding applied after it."""
    g = torch.Generator().manual_seed(C_ + S + stride)
    cg = C_ // 32
    x = torch.randn(B, C_, S, S, generator=g)
    w = torch.randn(C_, cg, 3, 3, generator=g) / (3 * cg ** 0.5)
    sc, sh = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.5
    q = _q(dt)
    xq = q(x)
    act = q(torch.relu(xq * sc[None, :, None, None] + sh[None, :, None, None]))
    ref = F.conv2d(act, q(w), None, stride, 1, 1, 32)
    cen = ref.mean(dim=(0, 2, 3)) + 0.05 * torch.randn(C_, generator=g) if centred else None      # centred storage: round(y - c)
    ref = q(ref - cen[None, :, None, None]) if centred else q(ref)
    cend = cen.to(dev) if centred else None
    cd = H.BF16 if dt == "bf16" else H.F32
    wp = pack(H, dt, H.PACK_GCONV3, w, dev)
    So = (S - 1) // stride + 1
    y = torch.empty(B, So, So, C_, dtype=_t(dt), device=dev)
    rows = H.lib().cvcl_gconv3x3_stats_rows(cd, B, S, S, C_, stride)
    st = stats_tensor(rows, C_, dev)
    xd, scd, shd = nhwc(xq).to(_t(dt)).to(dev), sc.to(dev), sh.to(dev)      # keep device operands alive
    H.check(H.lib().cvcl_gconv3x3(cd, H.ptr(xd), H.ptr(scd), H.ptr(shd), H.ptr(wp),
                                  H.ptr(y), H.ptr(st), rows, H.ptr(cend), B, S, S, C_, 32, stride, H.stream_ptr()), "gconv")
    torch.cuda.synchronize()
    assert maxrel(y.float(), nhwc(ref)) < (8e-3 if dt == "bf16" else 2e-5)
    check_stats(st, rows, y)


def test_gconv_fp32_direct_fallback(H, dev):
    """Shapes outside the LDS-tiled fp32 kernel's set (here 3 channels per group, C not a multiple of 64) take the direct kernel."""
    g = torch.Generator().manual_seed(11)
    B, C_, S, groups, stride = 2, 96, 12, 32, 2
    cg = C_ // groups
    x = torch.randn(B, C_, S, S, generator=g)
    w = torch.randn(C_, cg, 3, 3, generator=g) / (3 * cg ** 0.5)
    sc, sh = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.5
    ref = F.conv2d(torch.relu(x * sc[None, :, None, None] + sh[None, :, None, None]), w, None, stride, 1, 1, groups)
    So = (S - 1) // stride + 1
    y = torch.empty(B, So, So, C_, device=dev)
    rows = H.lib().cvcl_gconv3x3_stats_rows(H.F32, B, S, S, C_, stride)
    st = stats_tensor(rows, C_, dev)
    xd, scd, shd, wd = nhwc(x).to(dev), sc.to(dev), sh.to(dev), w.contiguous().to(dev)
    H.check(H.lib().cvcl_gconv3x3(H.F32, H.ptr(xd), H.ptr(scd), H.ptr(shd), H.ptr(wd), H.ptr(y), H.ptr(st), rows, None, B, S, S, C_,
                                  groups, stride, H.stream_ptr()), "gconv")
    assert maxrel(y, nhwc(ref)) < 2e-5
    check_stats(st, rows, y)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_add_relu_and_avgpool(H, dev, dt):
    g = torch.Generator().manual_seed(9)
    rows, Cn = 2 * 49, 2048
    q = _q(dt)
    raw, idn = q(torch.randn(rows, Cn, generator=g)), q(torch.randn(rows, Cn, generator=g))
    s1, b1 = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    s2, b2 = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    cd = H.BF16 if dt == "bf16" else H.F32
    rawd, idnd = raw.to(_t(dt)).to(dev), idn.to(_t(dt)).to(dev)              # keep device operands alive
    s1d, b1d, s2d, b2d = s1.to(dev), b1.to(dev), s2.to(dev), b2.to(dev)
    out = torch.empty(rows, Cn, dtype=_t(dt), device=dev)
    for with_ds in (False, True):
        ref = torch.relu(raw * s1 + b1 + (idn * s2 + b2 if with_ds else idn))
        H.check(H.lib().cvcl_bn_add_relu(cd, H.ptr(rawd), H.ptr(s1d), H.ptr(b1d), H.ptr(idnd),
                                         H.ptr(s2d) if with_ds else None, H.ptr(b2d) if with_ds else None, H.ptr(out),
                                         rows, Cn, H.stream_ptr()), "bn_add_relu")
        assert maxrel(out.float(), q(ref)) < (5e-3 if dt == "bf16" else 1e-6)
    # relu(bn(x)) in place (the pass that runs ahead of conv3)
    buf = rawd.clone()
    H.check(H.lib().cvcl_bn_relu_apply(cd, H.ptr(buf), H.ptr(s1d), H.ptr(b1d), H.ptr(buf), rows, Cn, H.stream_ptr()), "bn_relu_apply")
    assert maxrel(buf.float(), q(torch.relu(raw * s1 + b1))) < (5e-3 if dt == "bf16" else 1e-6)
    pooled = torch.empty(2, Cn, device=dev)
    H.check(H.lib().cvcl_avgpool(cd, H.ptr(out), H.ptr(pooled), 2, 49, Cn, H.stream_ptr()), "avgpool")
    assert maxrel(pooled, out.float().reshape(2, 49, Cn).mean(dim=1)) < 1e-5


def _load_oracle_params_into(model, p):
    sd = model.state_dict()
    for k, v in p.items():
        assert k in sd, k
        sd[k].copy_(v)


@pytest.mark.parametrize("dt,training", [("f32", True), ("f32", False), ("bf16", True), ("bf16", False)])
@pytest.mark.parametrize("B,S", [(2, 224), (3, 64)])
def test_trunk_vs_oracle(H, dev, dt, training, B, S):
    """Whole trunk (53 conv+BN, pools) through cvcl_resnext50_fwd vs the oracle; running statistics too."""
    from multimodal.resnext import ResNet
    p = O.resnext50_random_params(seed=1)
    g = torch.Generator().manual_seed(B * S)
    # non-trivial BN parameters / running stats so eval mode and the affine are exercised
    for k in list(p.keys()):
        if k.endswith("running_mean"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".weight"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
    x = torch.randn(B, 3, S, S, generator=g)
    stats_o = {}
    # bf16 stores every raw conv output centred (include/cvcl_hip.h "Centred storage"): on the batch means of a plain-storage
    # calibration pass in train mode, on the running means in eval mode; the oracle's storage-point emulation does the same
    centres = None
    if dt == "bf16":
        centres = O.resnext50_batch_means(p, x, _q(dt)) if training else "running_mean"
    pooled_o, fmap_o = O.resnext50_forward(p, x, training, _q(dt) if dt == "bf16" else None, stats_out=stats_o, centres=centres)
    model = ResNet()
    _load_oracle_params_into(model, p)
    model = model.to(dev)
    model.compute_dtype = _t(dt)
    model.train(training)
    for prm in model.parameters():
        prm.requires_grad_(False)
    pooled, fmap = model.trunk(x.to(dev))
    e_p, e_f = maxrel(pooled, pooled_o), maxrel(fmap.float(), fmap_o)
    cos = float(torch.nn.functional.cosine_similarity(pooled.cpu().flatten().double(), pooled_o.flatten().double(), dim=0))
    print(f"trunk {dt} train={training} B={B} S={S}: pooled rel err {e_p:.2e}, layer4 map rel err {e_f:.2e}, cos {cos:.5f}")
    assert fmap.shape == fmap_o.shape
    sd = model.state_dict()
    if dt == "bf16" and training:
        # A random-init ResNeXt with batch-statistic BN over a handful of samples is chaotic in bf16: one flipped bf16
        # rounding of a stored value spreads through every later BatchNorm.  The tolerance is therefore MEASURED, not assumed:
        # the oracle's own storage-point emulation with every convolution's input channels visited in reverse order (same
        # mathematics, other fp32 summation order) against itself.  The HIP trunk must be as close to the oracle as that
        # (x 3: a max over 2048 x B values of a heavy-tailed error), and the early layers' statistics, which the amplification
        # has not reached yet, must agree to bf16 precision.
        pooled_y, fmap_y = O.resnext50_forward(p, x, True, _q(dt), centres=centres, conv_fn=O.reordered_conv2d)
        y_p, y_f = maxrel(pooled_y, pooled_o), maxrel(fmap_y, fmap_o)
        y_cos = float(torch.nn.functional.cosine_similarity(pooled_y.flatten().double(), pooled_o.flatten().double(), dim=0))
        print(f"   yardstick (oracle vs reordered oracle): pooled {y_p:.2e}, map {y_f:.2e}, cos {y_cos:.5f}")
        assert e_p < 3 * y_p + 0.02 and e_f < 3 * y_f + 0.02 and 1 - cos < 3 * (1 - y_cos) + 1e-3
        for k, tol_k in (("bn1.running_mean", 2e-3), ("bn1.running_var", 2e-3), ("layer1.0.bn1.running_mean", 1e-2),
                         ("layer1.0.bn2.running_var", 2e-2), ("layer1.0.downsample.1.running_var", 2e-2)):
            assert maxrel(sd[k], stats_o[k]) < tol_k, k
    else:
        tol = 3e-2 if dt == "bf16" else 2e-4
        assert e_p < tol and e_f < tol
    if training:
        if dt == "f32":
            for k in ("bn1.running_mean", "layer1.0.bn2.running_var", "layer2.0.downsample.1.running_mean",
                      "layer4.2.bn3.running_var", "layer3.5.bn1.running_mean"):
                assert maxrel(sd[k], stats_o[k]) < 1e-4, k
        assert int(sd["layer4.2.bn3.num_batches_tracked"]) == 1
    else:
        assert torch.equal(sd["bn1.running_mean"].cpu(), p["bn1.running_mean"])
        assert int(sd["bn1.num_batches_tracked"]) == 0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_deferred_statistics_pass_is_the_in_place_pass(H, dev, dt):
    """cvcl_resnext50_fwd_deferred_stats + cvcl_resnext50_apply_moments (the form that lets two passes of a frozen trunk run on
    two streams) against cvcl_resnext50_fwd(training = 1): same outputs, and after three passes the same 53 x (running_mean,
    running_var, num_batches_tracked), bit for bit; the pass itself must leave the BatchNorm buffers untouched."""
    import copy
    from multimodal.resnext import ResNet, BN_MOMENTUM, BN_EPS
    torch.manual_seed(3)
    ref = ResNet().to(dev).train()
    ref.compute_dtype = _t(dt)
    for prm in ref.parameters():
        prm.requires_grad_(False)
    alt = copy.deepcopy(ref)
    lib, cd = H.lib(), H.cvcl_dtype(_t(dt))
    B, S = 3, 64
    arr, _keep = alt._packed_layers(cd, dev)
    nb = lib.cvcl_resnext50_workspace_bytes(cd, B, S, S)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    moments = torch.empty(lib.cvcl_resnext50_moments_floats(), dtype=torch.float32, device=dev)
    for i in range(3):
        x = torch.randn(B, 3, S, S, device=dev)
        pooled_r, fmap_r = ref.trunk(x)
        before = {k: v.clone() for k, v in alt.state_dict().items() if "running" in k or "tracked" in k}
        fmap = torch.empty(B, S // 32, S // 32, 2048, dtype=_t(dt), device=dev)
        pooled = torch.empty(B, 2048, dtype=torch.float32, device=dev)
        cen = ref.centres.frozen[1] if ref.centres.frozen else None      # bf16: the storage centres ref calibrated
        assert (cen is not None) == (dt == "bf16")
        H.check(lib.cvcl_resnext50_fwd_deferred_stats(cd, B, S, S, H.ptr(x), arr, len(arr), H.ptr(ws), nb, H.ptr(fmap), H.ptr(pooled),
                                                      BN_EPS, H.ptr(moments), H.ptr(cen), H.stream_ptr()), "deferred")
        after = alt.state_dict()
        assert all(torch.equal(v, after[k]) for k, v in before.items())          # the pass wrote no BatchNorm buffer
        H.check(lib.cvcl_resnext50_apply_moments(arr, len(arr), H.ptr(moments), BN_MOMENTUM, H.stream_ptr()), "apply")
        assert torch.equal(pooled, pooled_r) and torch.equal(fmap.permute(0, 3, 1, 2), fmap_r)
    sd_r, sd_a = ref.state_dict(), alt.state_dict()
    n = 0
    for k, v in sd_r.items():
        if "running" in k or "tracked" in k:
            assert torch.equal(v, sd_a[k]), k
            n += 1
    assert n == 53 * 3 and int(sd_a["layer4.2.bn3.num_batches_tracked"]) == 3
    with pytest.raises(H.CvclError):
        H.check(lib.cvcl_resnext50_fwd_deferred_stats(cd, B, S, S, H.ptr(x), arr, len(arr), H.ptr(ws), nb, H.ptr(fmap), H.ptr(pooled),
                                                      BN_EPS, None, None, H.stream_ptr()), "deferred")


def test_trunk_properties_full_batch(H, dev):
    """BASELINE batch (256 x 224 x 224, bf16): eval-mode per-sample independence (a sample's features do not
    depend on its batch-mates) and determinism (bit-identical reruns)."""
    from multimodal.resnext import ResNet
    torch.manual_seed(0)
    model = ResNet().to(dev).eval()
    model.compute_dtype = torch.bfloat16
    for prm in model.parameters():
        prm.requires_grad_(False)
    x = torch.randn(256, 3, 224, 224, device=dev)
    p1, f1 = model.trunk(x)
    p2, _ = model.trunk(x)
    assert torch.equal(p1, p2)
    p3, _ = model.trunk(x[100:104].contiguous())
    assert torch.equal(p1[100:104], p3)
    assert torch.isfinite(p1).all()
    model.train()
    p4, _ = model.trunk(x)
    p5, _ = model.trunk(x)
    assert torch.equal(p4, p5)                      # train-mode statistics are deterministic (no atomics)


@pytest.mark.parametrize("B,Hh,Ww", [(1, 224, 224), (5, 160, 160), (2, 256, 192)])
def test_trunk_other_shapes(H, dev, B, Hh, Ww):
    """Edge shapes: a single image (BN over one sample's pixels), odd batch, non-square / non-224 resolutions
    (multiples of 32), fp32 parity mode in both BN modes and bf16 eval vs the emulating oracle."""
    from multimodal.resnext import ResNet
    p = O.resnext50_random_params(seed=3)
    x = torch.randn(B, 3, Hh, Ww, generator=torch.Generator().manual_seed(B + Hh))
    model = ResNet()
    _load_oracle_params_into(model, p)
    model = model.to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)
    for training in (False, True):
        model.load_state_dict({k: v for k, v in p.items()}, strict=False)       # reset running statistics
        model.train(training)
        model.compute_dtype = torch.float32
        pooled_o, fmap_o = O.resnext50_forward(p, x, training)
        pooled, fmap = model.trunk(x.to(dev))
        assert fmap.shape == fmap_o.shape == (B, 2048, Hh // 32, Ww // 32)
        assert maxrel(pooled, pooled_o) < 5e-4 and maxrel(fmap.float(), fmap_o) < 5e-4, training
    model.eval()
    model.load_state_dict({k: v for k, v in p.items()}, strict=False)
    model.compute_dtype = torch.bfloat16
    pooled_b, _ = model.trunk(x.to(dev))
    pooled_q, _ = O.resnext50_forward(p, x, False, O.bf16_round)
    assert maxrel(pooled_b, pooled_q) < 3e-2


def test_trunk_rejects_bad_inputs(H, dev):
    from multimodal.resnext import ResNet
    model = ResNet().to(dev).eval()
    for prm in model.parameters():
        prm.requires_grad_(False)
    with pytest.raises(H.CvclError):
        model.trunk(torch.zeros(1, 3, 224, 224, device=dev, dtype=torch.float16))
    with pytest.raises(H.CvclError):
        model.trunk(torch.zeros(1, 3, 100, 100, device=dev))            # not a multiple of 32
    model.layer1[0].conv1.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError):                             # fine-tuning needs the trunk backward
        model.trunk(torch.zeros(1, 3, 224, 224, device=dev))
