"""GPU: the bf16 backward of the ResNeXt trunk (multimodal/trunk_train.py, --finetune_cnn) at the shapes it really runs at --
B = 256 images of 224 x 224 -- against float64 arithmetic on the very tensors each kernel saw (teacher-forced: the chaos of
the whole trunk's bf16 gradients does not enter).

At these sizes the kernels run other schedules than at the toy sizes of test_trunk_train_gpu.py: the grouped-conv weight
gradient gives each workgroup several (image, band) items, the BatchNorm backward runs at its capped partial-row grid, the
weight-gradient GEMMs contract over up to 3.2 M rows and the data-gradient GEMMs take the byte-stream kernels.

  * integer operands: every product and partial sum is an integer below 2^24, so any split or order of the fp32 sums is
    exact; weight gradients (fp32) must equal float64 bit for bit, bf16 data gradients must equal the bf16 rounding of the
    exact result.  The bound is stated per case.
  * BatchNorm: float64 reference from the stored bf16 tensor and the forward's own mean / rstd, per-channel bounds.
  * max pool: torch-CPU max_pool2d with indices (first arg-max wins), bit for bit.

References are float64 matmuls / einsums over tap-shifted views on the GPU (never F.conv2d on the GPU: MIOpen's algorithms
are not exact on integers), or torch-CPU in chunks of images."""
import gc

import pytest
import torch
import torch.nn.functional as F

from multimodal import _hip as H

pytestmark = pytest.mark.gpu

B = 256                                                   # C2's batch at 224 x 224: stem map 112^2, layer 1 at 56^2
EINVAL = -1                                               # include/cvcl_hip.h CVCL_EINVAL
BF = torch.bfloat16
F64 = torch.float64

# (layer, Cin of the layer, width, Cout, input size, stride of block 0)
LAYERS = [(1, 64, 128, 256, 56, 1), (2, 256, 256, 512, 56, 2), (3, 512, 512, 1024, 28, 2), (4, 1024, 1024, 2048, 14, 2)]


@pytest.fixture(autouse=True)
def _release(dev):
    """each case's tensors are gone (and their memory back with the driver) before the next case starts"""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ints(shape, lo, hi, seed, dev, dtype=BF):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).to(dtype)


def _exact_bf16(t64):
    """bf16 rounding (nearest even) of an exact float64 integer tensor whose values fit fp32 exactly (< 2^24)"""
    return t64.float().to(BF)


def _same(a, b):
    """equal values, shape and dtype (bit for bit but for the sign of a zero: a masked-out gradient is +0 here, -0 there)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ---- 1x1 convolutions: data gradient (bf16) and weight gradient (_gemm_tn, fp32) -----------------------------------------------
def _conv1x1_cases():
    cases = []
    for li, cin, width, cout, S, s in LAYERS:
        So = S // s
        cases += [(f"layer{li}.0.conv1", True, cin, width, S, 1),             # Conv1x1Skip (the block input also feeds the identity)
                  (f"layer{li}.0.conv3", False, width, cout, So, 1),
                  (f"layer{li}.0.downsample", False, cin, cout, S, s),        # stride 2 through cvcl_zero_stuff2 in layers 2-4
                  (f"layer{li}.1.conv1", True, cout, width, So, 1)]           # (conv3 of the later blocks: the shape of .0.conv3)
    return cases


@pytest.mark.parametrize("name,skip,K,N,S,stride", _conv1x1_cases(), ids=[c[0] for c in _conv1x1_cases()])
def test_conv1x1_grads_exact_fullsize(dev, name, skip, K, N, S, stride):
    """dX = dY W (Conv1x1: zero-stuffed dY at stride 2; Conv1x1Skip: + the identity's gradient d_skip, rounded twice) and
    dW = dY^T X (cvcl_gemm_tn over M = B S^2 rows) on operands in {-2..2}.
    Bounds: dW partial sums <= 4 M = 4 * 256 * 56^2 = 3 211 264 < 2^24;  dY W <= 4 N <= 8192, + d_skip <= 8194 < 2^24."""
    from multimodal.trunk_train import Conv1x1, Conv1x1Skip
    So = (S - 1) // stride + 1
    x = _ints((B, S, S, K), -2, 2, K + S, dev).requires_grad_()
    w = _ints((N, K, 1, 1), -2, 2, N + 1, dev, torch.float32).requires_grad_()
    dy = _ints((B, So, So, N), -2, 2, N + S + 2, dev)
    if skip:
        raw, _st, xv = Conv1x1Skip.apply(x, w)
        d_skip = _ints((B, S, S, K), -2, 2, K + 3, dev)
        torch.autograd.backward([raw, xv], [dy, d_skip])
    else:
        raw, _st = Conv1x1.apply(x, w, stride)
        raw.backward(dy)
    assert raw.shape == (B, So, So, N)
    W64 = w.detach().view(N, K).double()
    dy64 = dy.view(-1, N).double()
    xs = x.detach()[:, ::stride, ::stride].reshape(-1, K).double()          # the input pixels the kernel's output pixels read
    dw_ref = (dy64.t() @ xs).view(N, K, 1, 1).float()
    assert w.grad.dtype == torch.float32 and torch.equal(w.grad, dw_ref), name
    del xs, dw_ref
    dx_ref = torch.zeros(B, S, S, K, dtype=BF, device=dev)
    dx_ref[:, ::stride, ::stride] = _exact_bf16(dy64 @ W64).view(B, So, So, K)
    if skip:
        dx_ref = (dx_ref.float() + d_skip.float()).to(BF)                  # a bf16 + bf16 sum of integers < 2^24: exact in fp32
    assert _same(x.grad, dx_ref), name


@pytest.mark.parametrize("shape", [(2, 8, 8, 64, 128), (B, 56, 56, 256, 128)], ids=["small", "layer1.1.conv1"])
def test_conv1x1skip_fused_residual_is_gemm_plus_add(dev, shape):
    """Conv1x1Skip folds the identity's gradient into the data-gradient GEMM as its residual operand; its docstring promises
    dX = round(round(dY W) + d_skip), the same two roundings as the GEMM followed by a bf16 add -- bit for bit, on random
    (not integer) operands.  At the layer-1 shape (M = 802 816 >= 2^17 rows, contraction 128, N = 256) the separate GEMM takes
    the byte-stream kernel of pick_gemm_pro (which has no residual operand) and the fused one a tiled kernel."""
    from multimodal.trunk_train import Conv1x1Skip, _pack, _transpose
    Bn, S, _, K, N = shape
    g = torch.Generator(device=dev).manual_seed(K + N + S)
    x = torch.randn(Bn, S, S, K, generator=g, device=dev).to(BF).requires_grad_()
    w = (torch.randn(N, K, 1, 1, generator=g, device=dev) / K ** 0.5).requires_grad_()
    dy = torch.randn(Bn, S, S, N, generator=g, device=dev).to(BF)
    d_skip = torch.randn(Bn, S, S, K, generator=g, device=dev).to(BF)
    raw, _st, xv = Conv1x1Skip.apply(x, w)
    torch.autograd.backward([raw, xv], [dy, d_skip])
    M = Bn * S * S
    wq = _pack(w.detach(), H.PACK_DENSE, BF).view(BF).view(N, K)
    sep = H.gemm(dy.view(M, N), _transpose(wq))                            # round(dY W)
    ref = torch.empty_like(sep)
    H.check(H.lib().cvcl_add(H.cvcl_dtype(BF), H.ptr(sep), H.ptr(d_skip), H.ptr(ref), M * K, 0, H.stream_ptr()), "cvcl_add")
    assert _same(x.grad.view(M, K), ref)
    # the residual really is in there (a fused dX equal to the bare GEMM would mean d_skip was dropped)
    assert not torch.equal(x.grad.view(M, K), sep)


# ---- grouped 3x3 convolution: weight gradient (band kernel) and data gradient -----------------------------------------------------
def _gconv_cases():
    cases = []
    for li, _cin, width, _cout, S, s in LAYERS:
        if s == 2:
            cases.append((f"layer{li}.0.conv2", width, S, 2))
        cases.append((f"layer{li}.1.conv2", width, S // s, 1))           # (layer1.0.conv2 has the shape of layer1.1.conv2)
    return cases


def _gw_groups_and_min_items(S, C, stride):
    """workgroups per 128-channel slab of the band weight-gradient kernel, from its workspace ([slab][G][9 taps][4 waves][32][32]
    fp32 partial blocks), and a lower bound on its (image, band) items: a band of TH output rows keeps (TH - 1) * stride + 3 input
    rows of S + 2 pixels and TH rows of the 16-padded output row in at most 160 KB of LDS at 320 bytes per pixel"""
    nb = H.lib().cvcl_gconv3x3_wgrad_workspace_bytes(B, S, S, C, stride)
    slabs, blk = C // 128, 9 * 4 * 32 * 32 * 4
    assert nb % (slabs * blk) == 0, nb
    So = (S - 1) // stride + 1
    wo_pad = (So + 15) // 16 * 16
    th_max = max(th for th in range(1, So + 1) if (((th - 1) * stride + 3) * (S + 2) + th * wo_pad) * 320 <= 160 * 1024)
    return nb // (slabs * blk), B * -(-So // th_max)


@pytest.mark.parametrize("name,C,S,stride", _gconv_cases(), ids=[c[0] for c in _gconv_cases()])
def test_gconv3x3_grads_exact_fullsize(dev, name, C, S, stride):
    """GroupedConv3x3 (32 groups) backward on operands in {-2..2}:
      dW (cvcl_gconv3x3_wgrad, band kernel): sums over B Ho Wo <= 802 816 pixels of products <= 4: <= 3 211 264 < 2^24 -> exact fp32;
      dX (cvcl_gconv_weight_dgrad + cvcl_gconv3x3 on the zero-stuffed dY): <= 9 taps x 32 channels x 4 = 1152 -> bf16 of the exact sum.
      out (the forward cvcl_gconv3x3 itself, no prologue, at its full-batch schedule): the same bound, bf16 of the exact sum.
    The weight-gradient kernel must be in its multi-item regime: fewer workgroups per slab than (image, band) items."""
    from multimodal.trunk_train import GroupedConv3x3
    G, min_items = _gw_groups_and_min_items(S, C, stride)
    assert G < min_items, (G, min_items)                         # each workgroup accumulates several items
    cg = C // 32
    So = (S - 1) // stride + 1
    x = _ints((B, S, S, C), -2, 2, C + S, dev).requires_grad_()
    w = _ints((C, cg, 3, 3), -2, 2, C + 7, dev, torch.float32).requires_grad_()
    dy = _ints((B, So, So, C), -2, 2, C + S + 1, dev)
    out, _st = GroupedConv3x3.apply(x, w, stride)
    assert out.shape == dy.shape
    out.backward(dy)
    M = B * So * So
    dyg = dy.view(M, 32, cg).double().permute(1, 2, 0)                     # [group][co in group][pixel]
    xp = F.pad(x.detach(), (0, 0, 1, 1, 1, 1))                             # zero halo of the padding = 1 convolution
    dw_ref = torch.empty(C, cg, 3, 3, dtype=F64, device=dev)
    wg = w.detach().double().view(32, cg, cg, 3, 3)                          # [group][co][ci][ky][kx]
    dxp = torch.zeros(B, S + 2, S + 2, C, dtype=F64, device=dev)
    out_ref = torch.zeros(32, M, cg, dtype=F64, device=dev)                  # [group][pixel][co]
    for ky in range(3):
        for kx in range(3):
            rows = slice(ky, ky + stride * (So - 1) + 1, stride)
            cols = slice(kx, kx + stride * (So - 1) + 1, stride)
            xt = xp[:, rows, cols].reshape(M, 32, cg).double().permute(1, 0, 2)     # [group][pixel][ci]: the tap's input pixels
            dw_ref[:, :, ky, kx] = torch.bmm(dyg, xt).reshape(C, cg)
            out_ref += torch.bmm(xt, wg[:, :, :, ky, kx].transpose(1, 2))    # out[.., g, co] += X[tap pixel, g, ci] W[g, co, ci, tap]
            del xt
            # dX at the tap's input pixels += dY[.., g, co] W[g, co, ci, tap]
            dxp[:, rows, cols] += torch.bmm(dyg.transpose(1, 2), wg[:, :, :, ky, kx]).permute(1, 0, 2).reshape(B, So, So, C)
    assert _same(out.detach(), _exact_bf16(out_ref.permute(1, 0, 2).reshape(B, So, So, C))), name
    del out_ref
    assert torch.equal(w.grad, dw_ref.float()), name
    del dw_ref, dyg
    assert _same(x.grad, _exact_bf16(dxp[:, 1:S + 1, 1:S + 1])), name


def test_gconv3x3_wgrad_refuses_misaligned_operands(dev):
    """cvcl_gconv3x3_wgrad reads 16-byte chunks of x and dy: an operand one element off that alignment is refused on the host
    (CVCL_EINVAL + message), as cvcl_gemm_tn refuses it -- and nothing is launched: output and workspace keep their contents."""
    Bn, S, C = 2, 8, 128
    n = Bn * S * S * C
    lib = H.lib()
    nb = lib.cvcl_gconv3x3_wgrad_workspace_bytes(Bn, S, S, C, 1)
    buf_x = torch.zeros(n + 8, dtype=BF, device=dev)
    buf_d = torch.zeros(n + 8, dtype=BF, device=dev)
    dw = torch.full((C, C // 32, 3, 3), 7.0, device=dev)
    ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for x, dy in ((buf_x[1:n + 1], buf_d[:n]), (buf_x[:n], buf_d[1:n + 1])):
        assert (H.ptr(x) % 16 == 0) != (H.ptr(dy) % 16 == 0)
        rc = lib.cvcl_gconv3x3_wgrad(H.ptr(x), H.ptr(dy), H.ptr(dw), Bn, S, S, C, 32, 1, H.ptr(ws), nb, H.stream_ptr())
        assert rc == EINVAL
        assert "16-byte" in lib.cvcl_last_error().decode()
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((ws == 0xA5).all())


# ---- stem: im2col + TN GEMM over 3.2 M rows ---------------------------------------------------------------------------------------
def test_stem_wgrad_exact_fullsize(dev):
    """conv1 weight gradient (cvcl_stem_im2col + cvcl_gemm_tn, k_keep = 147) over P = 256 * 112^2 = 3 211 264 patch rows, on
    integer images in {-2..2} (exact after the bf16 cast) and dY in {-2..2}: partial sums <= 4 P = 12 845 056 < 2^24."""
    from multimodal.trunk_train import StemConv
    P = B * 112 * 112
    x = _ints((B, 3, 224, 224), -2, 2, 11, dev, torch.float32)
    w = _ints((64, 3, 7, 7), -2, 2, 12, dev, torch.float32).requires_grad_()
    dy = _ints((B, 112, 112, 64), -2, 2, 13, dev)
    out, _st = StemConv.apply(x, w, BF)
    assert out.shape == dy.shape
    out.backward(dy)
    xp = F.pad(x.double(), (3, 3, 3, 3))
    col = torch.empty(P, 3, 7, 7, dtype=F64, device=dev)                   # the patch matrix, columns in OIHW weight order
    for ky in range(7):
        for kx in range(7):
            col[:, :, ky, kx] = xp[:, :, ky:ky + 223:2, kx:kx + 223:2].permute(0, 2, 3, 1).reshape(P, 3)
    del xp
    ref = (dy.view(P, 64).double().t() @ col.view(P, 147)).view(64, 3, 7, 7)
    assert torch.equal(w.grad, ref.float())


# ---- BatchNorm backward, teacher-forced --------------------------------------------------------------------------------------------
def _bn_data(rows_shape, C, centred, seed, dev):
    """y with per-channel means / spreads over a wide range (one channel 100x smaller than the rest); stored as raw = round(y - c)
    with a centre c near the batch mean, or as raw = round(y) (mean within a few spreads)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    sig = torch.exp(torch.randn(C, generator=g, device=dev) * 0.8) * 0.5
    sig[C // 3] *= 0.01
    mu = sig * (torch.rand(C, generator=g, device=dev) * 100 - 50 if centred else torch.rand(C, generator=g, device=dev) * 8 - 4)
    z = torch.randn(*rows_shape, C, generator=g, device=dev)
    y = mu + sig * z
    c = (mu + 0.3 * sig * torch.randn(C, generator=g, device=dev)) if centred else None
    raw = (y - c).to(BF) if centred else y.to(BF)
    # an upstream gradient with a per-channel mean and a part along z: sum(dy) and sum(dy xhat) are far from zero (a dropped
    # slice of rows moves them by its share, not by sqrt of it)
    dy = (torch.randn(z.shape, generator=g, device=dev) + torch.randn(C, generator=g, device=dev)
          + torch.randn(C, generator=g, device=dev) * z).to(BF)
    gamma = torch.rand(C, generator=g, device=dev) + 0.5
    beta = torch.randn(C, generator=g, device=dev) * 0.3
    idn = torch.randn(*rows_shape, C, generator=g, device=dev).to(BF)
    return raw, c, dy, gamma, beta, idn


BN_CASES = [("relu", (B, 56, 56), 128), ("relu", (B, 112, 112), 64), ("plain", (B, 56, 56), 256), ("plain", (B, 112, 112), 64),
            ("tail", (B, 56, 56), 256), ("tail", (B, 112, 112), 64)]


@pytest.mark.parametrize("centred", [False, True], ids=["plain_storage", "centred"])
@pytest.mark.parametrize("kind,rows_shape,C", BN_CASES, ids=[f"{k}-{r[1]}x{r[2]}x{c}" for k, r, c in BN_CASES])
def test_batchnorm_backward_teacher_forced_fullsize(dev, kind, rows_shape, C, centred):
    """BatchNormTrain (ReLU on / off) and BnAddRelu at 802 816 and 3 211 264 rows, stored plainly or centred.  Reference in
    float64 from the stored bf16 raw (+ c) and the forward's own batch mean / rstd; the ReLU mask from the kernel's own forward
    output (which must agree with the float64 pre-activation except within one fp32 ulp of 0).  dbeta, dgamma and dx are
    checked per channel, against bounds scaled by that channel's sum |g|, sum |g xhat| and the size of the fp32 terms of dx."""
    from multimodal.trunk_train import BatchNormTrain, BnAddRelu
    rows = rows_shape[0] * rows_shape[1] * rows_shape[2]
    cap = 512 // max(1, (C // 8) // 256)                                   # bn_bwd_rows: 512 / (channel-chunk blocks)
    assert H.lib().cvcl_bn_bwd_partial_rows(H.cvcl_dtype(BF), rows, C) == cap
    raw, c, dy, gamma, beta, idn = _bn_data(rows_shape, C, centred, C + rows_shape[1] + int(centred), dev)
    raw.requires_grad_()
    gamma.requires_grad_()
    beta.requires_grad_()
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    c_track = None if c is None else c.clone()                             # the forward moves it to this batch's mean of y
    if kind == "tail":
        idn.requires_grad_()
        out = BnAddRelu.apply(raw, None, gamma, beta, rm, rv, nbt, idn, c_track)
        _raw, _out, mean, rstd, _g = out.grad_fn.saved_tensors
        dx, dgamma, dbeta, didn = torch.autograd.grad(out, [raw, gamma, beta, idn], dy)
    else:
        out = BatchNormTrain.apply(raw, None, gamma, beta, rm, rv, nbt, kind == "relu", c_track)
        _raw, _scale, _shift, mean, rstd, _g = out.grad_fn.saved_tensors
        dx, dgamma, dbeta = torch.autograd.grad(out, [raw, gamma, beta], dy)
    n = rows
    r64 = raw.detach().reshape(n, C).double()
    # the forward's batch moments are those of the stored tensor, within fp32-summation error of float64
    ms = r64.square().mean(0)
    var = (r64 - r64.mean(0)).square().mean(0) + 1e-5
    assert bool(((mean.double() - r64.mean(0)).abs() <= 1e-5 * ms.sqrt()).all()), "mean"
    assert bool(((rstd.double() * var.sqrt() - 1).abs() <= 1e-4 * ms / var + 1e-6).all()), "rstd"
    # teacher-forced reference: y = raw + c, xhat = (y - mean of y) rstd with the forward's own moments (mean of y = mean + c)
    cc = 0.0 if c is None else c.double()
    xhat = (r64 + cc - (mean.double() + cc)) * rstd.double()
    g64 = dy.reshape(n, C).double()
    if kind != "plain":
        # the mask is the kernel's own forward decision; it must be the sign of the exact pre-activation of the forward's own
        # affine (bit-identical scale / shift from the same statistics pass), but within one fp32 ulp of the summed terms of 0
        from multimodal.trunk_train import _bn_forward_stats
        sc, sh, _m, _r = _bn_forward_stats(raw.detach(), None, gamma.detach(), beta.detach(), torch.zeros(C, device=dev),
                                           torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev),
                                           None if c is None else c.clone())
        pre = r64 * sc.double() + sh.double()
        mag = (r64 * sc.double()).abs() + sh.double().abs()
        if kind == "tail":
            i64 = idn.detach().reshape(n, C).double()
            pre, mag = pre + i64, mag + i64.abs()
        mask = out.detach().reshape(n, C) > 0
        sure = pre.abs() > 2.0 ** -23 * mag
        assert bool((mask == (pre > 0))[sure].all()), "mask"
        del pre, mag, sure
        g64 = g64 * mask
    if kind == "tail":                                                     # the identity's gradient is g = dy * mask, exactly
        assert _same(didn.reshape(n, C), g64.to(BF))
    gx = g64 * xhat
    db_ref, dg_ref = g64.sum(0), gx.sum(0)
    sum_g, sum_gx = g64.abs().sum(0), gx.abs().sum(0)
    del gx
    assert bool(((dbeta.double() - db_ref).abs() <= 1e-4 * sum_g).all()), "dbeta"
    assert bool(((dgamma.double() - dg_ref).abs() <= 1e-4 * sum_gx).all()), "dgamma"
    # dx = gamma rstd (g - dbeta / n - xhat dgamma / n); the kernel evaluates k1 g + k2 raw + k3 in fp32 with k1 = gamma rstd,
    # k2 = -k1 rstd dgamma / n, k3 = -k1 dbeta / n - k2 mean from its fp32 dgamma / dbeta: bound by the size of those terms
    k1 = gamma.detach().double() * rstd.double()
    k2 = -k1 * rstd.double() * dg_ref / n
    k3 = -k1 * db_ref / n - k2 * mean.double()
    terms = (k1 * g64.abs().amax(0) + k2.abs() * r64.abs().amax(0) + k3.abs()
             + k1 * (sum_g + xhat.abs().amax(0) * sum_gx) / n)
    dx_ref = k1 * (g64 - db_ref / n - xhat * dg_ref / n)
    err = (dx.reshape(n, C).double() - dx_ref).abs() - 2.0 ** -8 * dx_ref.abs()             # (bf16 rounding of the result)
    assert bool((err.amax(0) <= 2e-5 * terms).all()), "dx"


# ---- max pool -----------------------------------------------------------------------------------------------------------------------
def test_maxpool_backward_fullsize_bit_exact(dev):
    """cvcl_maxpool3x3s2_idx on the stem's output 256 x 112 x 112 x 64: forward and backward bit for bit against torch-CPU
    max_pool2d with indices (first arg-max in window order wins -- inputs in {-2..2}, so ties are everywhere); dY in {-8..8}:
    an input pixel collects at most 4 windows' gradients, |sum| <= 32, exact in bf16."""
    from multimodal.trunk_train import MaxPool3x3s2
    x = _ints((B, 112, 112, 64), -2, 2, 21, dev).requires_grad_()
    dy = _ints((B, 56, 56, 64), -8, 8, 22, dev)
    out = MaxPool3x3s2.apply(x)
    out.backward(dy)
    xc, dyc, outc, dxc = x.detach().cpu(), dy.cpu(), out.detach().cpu(), x.grad.cpu()
    for b0 in range(0, B, 32):
        a = xc[b0:b0 + 32].permute(0, 3, 1, 2).double().requires_grad_()
        p, _idx = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        p.backward(dyc[b0:b0 + 32].permute(0, 3, 1, 2).double())
        assert _same(outc[b0:b0 + 32], p.detach().permute(0, 2, 3, 1).to(BF))
        assert _same(dxc[b0:b0 + 32], a.grad.permute(0, 2, 3, 1).to(BF))
