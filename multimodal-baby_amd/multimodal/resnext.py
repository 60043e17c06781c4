"""ResNeXt-50 32x4d with torchvision's module tree / state_dict keys, computed by libcvcl_hip.

The reference gets this network from ``torchvision.models.resnext50_32x4d``
(multimodal/multimodal.py:155-158, multimodal/utils.py:207-209 in the reference).  Here the
``nn.Conv2d`` / ``nn.BatchNorm2d`` children are *parameter containers only* (same names, shapes and
init as torchvision, so checkpoints interchange); ``forward`` hands their tensors to
``cvcl_resnext50_fwd`` which enqueues the whole trunk as hand-written HIP kernels.  There is no
PyTorch-op fallback: CPU tensors raise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import torch
import torch.nn as nn

from . import _hip as H
from . import ops
from .trunk_runtime import TrunkRuntime, fingerprint, strip

LAYERS = (3, 4, 6, 3)
GROUPS, WIDTH_PER_GROUP = 32, 4
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        width = int(planes * (WIDTH_PER_GROUP / 64.0)) * GROUPS
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=GROUPS, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):  # pragma: no cover - blocks are never run one by one
        raise H.CvclError("ResNeXt blocks are parameter containers; run the whole trunk through ResNet.forward")


class _Stage(nn.Sequential):
    """layer{1..4}: holds the Bottlenecks; called with the already-computed stage output so that
    forward hooks registered on it (the reference's ``Hook(model.layer4)``, attention_maps.py:83-101)
    observe the feature map exactly as with torchvision."""

    def forward(self, feature_map):
        return feature_map


class StorageCentres:
    """Centred storage of the raw convolution outputs (include/cvcl_hip.h "Centred storage"): the centres a ResNet holds.

    A raw conv output y whose per-channel batch mean is large next to its spread loses precision when it is rounded to bf16
    before BatchNorm subtracts the mean.  BatchNorm(y - c) == BatchNorm(y), so the kernels store round(y - c) with c close to
    the batch mean.  The frozen trunk takes c from ONE calibration pass -- the batch means of the first train-mode batch it
    sees after its weights (re)appeared -- and keeps it: a forward pass stays a pure function of (input, weights, BatchNorm
    buffers, centres), whatever the stream schedule.  c only has to be within ~sigma of the batch mean, which a stationary
    input distribution guarantees; ``reset()`` drops it (e.g. after a change of data distribution).
    Eval mode centres on the running means (the library's default for centres == NULL).  The fine-tuning twin
    (trunk_train) tracks instead: its weights move every step, so each layer's c follows the previous step's batch mean.
    $CVCL_CENTRED_STORAGE=0 switches the whole mechanism off (plain storage, the round-2 numerics; ResNet.centred_storage).

    The class launches nothing: ``calibrated`` is handed the calibration pass as a callable."""

    def __init__(self):
        self.frozen = None                  # (weights key, [53, 2048] f32, ready event or None): calibrated, frozen path
        self.restored = None                # "frozen" centres of a checkpoint, not yet adopted by a pass
        self.tracked = None                 # [53, 2048] f32 on the device: fine-tuning path
        self.tracked_restored = None        # "tracking" centres of a checkpoint, not yet adopted
        self.sync_pending = False

    def reset(self):
        """Forget the calibrated and the tracked centres.  Data parallel: all ranks call it, and all ranks' next train-mode pass
        adopts rank 0's new calibration (``request_sync``)."""
        self.frozen = self.restored = self.tracked = self.tracked_restored = None
        from . import parallel
        if parallel.is_distributed():
            self.request_sync()

    def request_sync(self):
        """Data parallel: ask the NEXT ``calibrated`` call to take part in one broadcast of rank 0's storage centres, whatever this
        replica's own state says (hit, restored from a checkpoint, freshly calibrated).  Raised only at rank-synchronous points --
        ``DataParallelEngine.attach`` and ``reset`` -- so either every rank enters the broadcast or none does: the decision never
        depends on a rank's local state (a checkpoint resumed on some ranks only, a weight re-allocated on one rank, a rank-local
        extra forward).  A miss WITHOUT a pending request recalibrates locally and talks to nobody."""
        self.sync_pending = True

    def export(self):
        """Checkpoint form (CPU tensors) {"frozen", "tracking"}, or None when there are none yet."""
        out = {}
        if self.frozen is not None:
            if self.frozen[2] is not None:
                self.frozen[2].synchronize()
            out["frozen"] = self.frozen[1].detach().cpu()
        elif self.restored is not None:
            out["frozen"] = self.restored.detach().cpu()
        if self.tracked is not None:
            out["tracking"] = self.tracked.detach().cpu()
        return out or None

    def import_(self, state):
        """Adopt what ``export`` saved: the next train-mode pass uses it instead of calibrating (whatever the weights' new storage
        addresses are), so a resumed bf16 run evaluates the same forward function as the run that saved it.  A checkpoint carries
        rank 0's centres (the ones every replica of a data-parallel run holds after the broadcast at its first step); on resume
        ``DataParallelEngine.attach`` requests the same broadcast again, so the replicas agree even when only some ranks restored."""
        self.frozen = self.tracked = None
        self.restored = state["frozen"].clone() if state.get("frozen") is not None else None
        self.tracked_restored = state["tracking"].clone() if state.get("tracking") is not None else None

    def tracking(self, device):
        t = self.tracked
        if t is None or t.device != device:
            pend, self.tracked_restored = self.tracked_restored, None
            t = self.tracked = pend.to(device) if pend is not None else torch.zeros(53, 2048, dtype=torch.float32, device=device)
        return t

    def calibrated(self, x, key, calibrate):
        """-> [53, 2048] f32 centres for a train-mode pass over ``x``'s distribution with the weights ``key``: the cached ones, the
        restored ones (restored wins over calibrating), or ``calibrate()``'s."""
        from . import parallel
        sync = self.sync_pending and parallel.is_distributed()
        hit = self.frozen
        if hit is not None and hit[0] == key:
            if hit[2] is not None:
                torch.cuda.current_stream(x.device).wait_event(hit[2])     # (calibrated on another trunk stream)
            if not sync:
                return hit[1]
            centres = hit[1]
        else:
            pend, self.restored = self.restored, None
            if pend is not None:                                  # restored from a checkpoint: no calibration pass
                centres = pend.to(device=x.device, dtype=torch.float32).contiguous()
                if not sync:
                    self.frozen = (key, centres, None)
                    return centres
            else:
                centres = calibrate()
        if sync:
            # data parallel: every replica must evaluate the SAME bf16 forward function, so rank 0's centres are adopted by all (a
            # centre only has to be within ~sigma of a rank's batch mean; the ranks see shards of one distribution).  Every rank is
            # here: the request was raised at a rank-synchronous point (request_sync), not by this rank's cache state
            self.sync_pending = False
            centres = parallel.broadcast_from_rank0(centres.clone() if hit is not None and centres is hit[1] else centres)
        ready = None
        if x.is_cuda:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(x.device))
        self.frozen = (key, centres, ready)
        return centres


class ResNet(nn.Module):
    def __init__(self, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), LAYERS), start=1):
            mods = []
            for bi in range(blocks):
                stride = 2 if (li > 1 and bi == 0) else 1
                ds = None
                if bi == 0:
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
                mods.append(Bottleneck(inplanes, planes, stride, ds))
                inplanes = planes * 4
            setattr(self, f"layer{li}", _Stage(*mods))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():                       # torchvision's init (zero_init_residual=False)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.compute_dtype = torch.float32             # torch.bfloat16 = perf mode
        # products of the trunk's convolutions when compute_dtype is fp32: "exact" (fp32 MFMA, the parity mode) or "split"
        # (split-bf16 parts on the bf16 MFMA, CVCL_F32X3: the "32-split" precision; storage stays fp32)
        self.trunk_arithmetic = "exact"
        self.runtime = TrunkRuntime(defers=True)       # never pickled: packed weights, workspaces, trunk stream, callback
        self.centres = StorageCentres()                # never pickled either (checkpoints carry export_centres())

    # ---- (conv, bn) pairs in torchvision state_dict order -----------------------------------
    def conv_bn_pairs(self):
        pairs = [(self.conv1, self.bn1, H.PACK_STEM7)]
        for li in (1, 2, 3, 4):
            for blk in getattr(self, f"layer{li}"):
                pairs.append((blk.conv1, blk.bn1, H.PACK_DENSE))
                pairs.append((blk.conv2, blk.bn2, H.PACK_GCONV3))
                pairs.append((blk.conv3, blk.bn3, H.PACK_DENSE))
                if blk.downsample is not None:
                    pairs.append((blk.downsample[0], blk.downsample[1], H.PACK_DENSE))
        return pairs

    def _packed_layers(self, dt: int, device):
        """Re-lay-out conv weights for the kernels (once per weight version) and build the C array."""
        pairs = self.conv_bn_pairs()
        key = fingerprint([c.weight for c, _, _ in pairs], dt, str(device), *(b.running_mean.data_ptr() for _, b, _ in pairs))
        return self.runtime.cache.get("pack", key, lambda: self._pack_layers(pairs, dt, device))

    def _pack_layers(self, pairs, dt, device):
        lib = H.lib()
        arr = (H.ConvBnParams * len(pairs))()
        keep = []
        for i, (conv, bn, kind) in enumerate(pairs):
            w = conv.weight.detach()
            cout, cing, k, _ = w.shape
            nb = lib.cvcl_packed_weight_bytes(dt, kind, cout, cing, k)
            buf = torch.empty(nb, dtype=torch.uint8, device=device)
            H.check(lib.cvcl_pack_conv_weight(dt, kind, H.ptr(w.contiguous(), torch.float32), H.ptr(buf), cout, cing, k,
                                              H.stream_ptr()), "cvcl_pack_conv_weight")
            keep.append(buf)
            arr[i].w = buf.data_ptr()
            arr[i].gamma = H.ptr(bn.weight.detach(), torch.float32)
            arr[i].beta = H.ptr(bn.bias.detach(), torch.float32)
            arr[i].running_mean = H.ptr(bn.running_mean, torch.float32)
            arr[i].running_var = H.ptr(bn.running_var, torch.float32)
            arr[i].num_batches_tracked = H.ptr(bn.num_batches_tracked, torch.int64)
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()   # packed once, then read by every stream that runs the trunk
        return arr, keep

    # ---- centred storage: StorageCentres (above) under the names the callers know ------------------------------------------
    def recalibrate_centres(self):
        self.centres.reset()                             # (data parallel: a collective call)

    def request_centre_sync(self):
        self.centres.request_sync()

    def export_centres(self):
        return self.centres.export()

    def import_centres(self, state):
        self.centres.import_(state)

    def centred_storage(self) -> bool:
        return os.environ.get("CVCL_CENTRED_STORAGE", "1") != "0" and self.compute_dtype == torch.bfloat16

    def tracking_centres(self, device):
        """[53, 2048] f32 centres of the fine-tuning path, updated in place by every BatchNorm forward (trunk_train)."""
        return self.centres.tracking(device) if self.centred_storage() else None

    def trunk(self, x: torch.Tensor, defer_wait: bool = False, bn_groups: int | None = None):
        """conv1 .. layer4 + avgpool.  -> (pooled [B,2048] f32, layer4 map as a logical NCHW view).  With a trunk stream and
        ``defer_wait`` the result is a handle for ``self.runtime.stream.wait`` (the caller's stream has not waited yet).
        ``bn_groups=G`` in train mode: every BatchNorm normalises each consecutive group of G images on that group's own batch
        statistics (``cvcl_resnext50_fwd_grouped``; running statistics untouched) -- each group's outputs are those of a
        train-mode pass over its G images alone.  In eval mode the running statistics serve every image and G changes nothing."""
        if bn_groups is not None and self.training:
            return self._trunk_grouped(x, int(bn_groups))
        if torch.is_grad_enabled() and any(p.requires_grad for c, b, _ in self.conv_bn_pairs() for p in (c.weight, b.weight, b.bias)):
            if self.trunk_dtype() == H.F32X3:
                raise H.CvclError("--finetune_cnn is not available in the 32-split precision (use 32 or bf16)")
            from .trunk_train import trunk_train       # --finetune_cnn: differentiable twin (saves activations)
            return trunk_train(self, x)
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise H.CvclError(f"expected NCHW fp32 images, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        ts = self.runtime.stream
        if ts is not None and x.is_cuda:                  # frozen trunk on its own stream (H.TrunkStream)
            handle = ts.launch(lambda slot: self._trunk_launch(x, slot), x)
            if defer_wait:
                return handle
            return ts.wait(handle)
        return self._trunk_launch(x)

    @contextlib.contextmanager
    def grouped_bn(self, bn_groups: int):
        """``with model.grouped_bn(G): logits = model(imgs)`` -- forward with ``trunk(x, bn_groups=G)`` (the linear probe's
        trial scoring: each G-image trial normalised on its own batch statistics, as the reference's train-mode model does)."""
        rt = self.runtime
        prev, rt.bn_groups = rt.bn_groups, int(bn_groups)
        try:
            yield self
        finally:
            rt.bn_groups = prev

    def _trunk_grouped(self, x, G):
        dt = self.trunk_dtype()
        if dt == H.BF16:
            raise H.CvclError("grouped train-mode BatchNorm (bn_groups) is available in the 32 and 32-split precisions, not bf16")
        if torch.is_grad_enabled() and any(p.requires_grad for c, b, _ in self.conv_bn_pairs() for p in (c.weight, b.weight, b.bias)):
            raise H.CvclError("bn_groups runs the frozen trunk only (no --finetune_cnn backward)")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise H.CvclError(f"expected NCHW fp32 images, got {tuple(x.shape)} {x.dtype}")
        B, _, Hh, Ww = x.shape
        if G < 1 or B % G:
            raise H.CvclError(f"bn_groups={G} does not divide the batch of {B} images")
        x = x.contiguous()
        lib = H.lib()
        with torch.no_grad():
            arr, _keep = self._packed_layers(dt, x.device)
            nb = lib.cvcl_resnext50_fwd_grouped_workspace_bytes(dt, B, Hh, Ww, G)
            ws = self.runtime.workspace(nb, x.device, "grouped")
            fmap = torch.empty(B, Hh // 32, Ww // 32, 2048, dtype=torch.float32, device=x.device)
            pooled = torch.empty(B, 2048, dtype=torch.float32, device=x.device)
            H.check(lib.cvcl_resnext50_fwd_grouped(dt, B, Hh, Ww, G, H.ptr(x), arr, len(arr), H.ptr(ws), nb, H.ptr(fmap), H.ptr(pooled),
                                                   BN_EPS, H.stream_ptr()), "cvcl_resnext50_fwd_grouped")
        return pooled, fmap.permute(0, 3, 1, 2)

    def enable_trunk_stream(self, device, inputs="caller", stream=None, n_streams=None):
        """Run the frozen trunk on a stream of its own so it overlaps the previous step's trainable tail (see H.TrunkStream).
        n_streams = 2 (the default; $CVCL_TRUNK_STREAMS overrides): consecutive passes alternate between two streams and also
        overlap each other -- each has its own workspace, and the BatchNorm running statistics are updated in pass order by
        ``cvcl_resnext50_apply_moments`` (same values as the one-stream schedule, bit for bit)."""
        if n_streams is None:
            n_streams = 1 if stream is not None else int(os.environ.get("CVCL_TRUNK_STREAMS", "2"))
        return self.runtime.set_stream(H.TrunkStream(device, inputs, stream, n_streams) if inputs else None)

    def trunk_dtype(self) -> int:
        """The library dtype the trunk forward runs in: compute_dtype's, or CVCL_F32X3 for fp32 storage with split products."""
        if self.compute_dtype == torch.float32 and self.trunk_arithmetic == "split":
            return H.F32X3
        return H.cvcl_dtype(self.compute_dtype)

    def _trunk_launch(self, x, slot=None):
        B, _, Hh, Ww = x.shape
        dt = self.trunk_dtype()
        lib = H.lib()
        with torch.no_grad():
            arr, _keep = self._packed_layers(dt, x.device)
            nb = lib.cvcl_resnext50_workspace_bytes(dt, B, Hh, Ww)
            rt = self.runtime
            ts = rt.stream
            piped = slot is not None and ts is not None and ts.n_streams > 1    # passes on two streams: scratch per stream
            sidx = ts.stream_index if piped else None
            ws = rt.workspace(nb, x.device, sidx)

            def outputs():
                return (torch.empty(B, Hh // 32, Ww // 32, 2048, dtype=self.compute_dtype, device=x.device),
                        torch.empty(B, 2048, dtype=torch.float32, device=x.device))
            # (side-stream mode: a ring of persistent output sets, H.TrunkStream.launch)
            fmap, pooled = outputs() if slot is None else rt.buffer(("out", slot, B, Hh, Ww, self.compute_dtype, str(x.device)), outputs)

            def batch_means():
                # the calibration pass: plain storage, train mode, leaves every layer's batch mean behind, touches no BatchNorm buffer
                moments = torch.empty(lib.cvcl_resnext50_moments_floats(), dtype=torch.float32, device=x.device)
                f, p = outputs()
                H.check(lib.cvcl_resnext50_fwd_deferred_stats(dt, B, Hh, Ww, H.ptr(x), arr, len(arr), H.ptr(ws), nb, H.ptr(f), H.ptr(p),
                                                              BN_EPS, H.ptr(moments), None, H.stream_ptr()), "cvcl_resnext50_fwd_deferred_stats")
                return moments.view(53, 2, 2048)[:, 0, :].contiguous()
            centred = self.training and self.centred_storage()
            centres = self.centres.calibrated(x, rt.cache.slots["pack"][0], batch_means) if centred else None
            if piped and self.training:
                # the pass leaves its batch moments behind; the 53 running-statistics updates run as one launch behind the
                # previous pass's (other stream), so they are applied in pass order with the one-stream arithmetic
                moments = rt.buffer(("moments", sidx, str(x.device)), lambda: torch.empty(
                    lib.cvcl_resnext50_moments_floats(), dtype=torch.float32, device=x.device))
                H.check(lib.cvcl_resnext50_fwd_deferred_stats(dt, B, Hh, Ww, H.ptr(x), arr, len(arr), H.ptr(ws), nb, H.ptr(fmap),
                                                              H.ptr(pooled), BN_EPS, H.ptr(moments), H.ptr(centres), H.stream_ptr()),
                        "cvcl_resnext50_fwd_deferred_stats")
                cur = torch.cuda.current_stream(x.device)
                if rt.ema_done is not None:
                    cur.wait_event(rt.ema_done)
                H.check(lib.cvcl_resnext50_apply_moments(arr, len(arr), H.ptr(moments), BN_MOMENTUM, H.stream_ptr()),
                        "cvcl_resnext50_apply_moments")
                rt.ema_done = torch.cuda.Event()
                rt.ema_done.record(cur)
            else:
                if rt.ema_done is not None and x.is_cuda:    # this pass reads / updates the running statistics in place: behind
                    torch.cuda.current_stream(x.device).wait_event(rt.ema_done)     # the last deferred update, whatever stream ran it
                # (eval mode: centres None = the library centres every stored tensor on its running mean)
                H.check(lib.cvcl_resnext50_fwd(dt, B, Hh, Ww, int(self.training), H.ptr(x), arr, len(arr), H.ptr(ws), nb,
                                               H.ptr(fmap), H.ptr(pooled), BN_MOMENTUM, BN_EPS, H.ptr(centres), H.stream_ptr()),
                        "cvcl_resnext50_fwd")
        return pooled, fmap.permute(0, 3, 1, 2)

    # the runtime holds ctypes arrays / device buffers / streams: never pickled (save_hyperparameters pickles whole encoder modules)
    def __getstate__(self):
        return strip(self.__dict__, "runtime", "centres")       # (__dict__: the instance's own state is what pickles)

    def __setstate__(self, d):
        # (objects pickled by torchvision lack the two settings; a pickle of an earlier version carries cache keys: dropped)
        self.__dict__.update({"compute_dtype": torch.float32, "trunk_arithmetic": "exact", **strip(d, "runtime", "centres")})
        self.runtime, self.centres = TrunkRuntime(defers=True), StorageCentres()

    def forward(self, x):
        rt = self.runtime
        ts, G = rt.stream, rt.bn_groups
        # (the batch path keeps its call exactly: callers may stand a plain function in for ``trunk``)
        out = self.trunk(x, defer_wait=True) if G is None else self.trunk(x, defer_wait=True, bn_groups=G)
        if rt.pre_head_callback is not None:
            rt.pre_head_callback()                       # deferred all-reduce wait + optimizer step of the previous step
        if ts is not None and isinstance(out, tuple) and len(out) == 2 and isinstance(out[1], torch.cuda.Event):
            out = ts.wait(out)                           # (with a trunk stream the update above overlapped the trunk)
        pooled, fmap = out
        # fire the forward hooks registered on layer4 (the reference's Hook(model.layer4)); done by hand so that it
        # also works when layer4 is a plain nn.Sequential unpickled from a torchvision-built checkpoint
        for hook in list(self.layer4._forward_hooks.values()):
            hook(self.layer4, (fmap,), fmap)
        if fmap.requires_grad and pooled.grad_fn is None and torch.is_grad_enabled():
            # a hook asked for the map's gradient (Grad-CAM: attention_maps.gradCAM) and the frozen trunk's pooled vector is not
            # connected to it: route it through the avgpool's backward so the gradient reaches the map
            pooled = _PooledFromMap.apply(pooled, fmap)
        if isinstance(self.fc, nn.Linear):
            return ops.linear_f32(pooled, self.fc.weight, self.fc.bias)
        return self.fc(pooled)                           # e.g. nn.Identity (utils.build_dino_mugs)


class _PooledFromMap(torch.autograd.Function):
    """The frozen trunk's adaptive avgpool as autograd sees it: forward hands back the trunk's own pooled vector unchanged, backward
    is d_map[n, p, c] = d_pooled[n, c] / hw (cvcl_avgpool_bwd) in the map's dtype and NHWC storage, returned as the map's NCHW view."""

    @staticmethod
    def forward(ctx, pooled, fmap):
        ctx.map_shape, ctx.map_dtype = tuple(fmap.shape), fmap.dtype
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        B, C, Hh, Ww = ctx.map_shape
        d_pooled = d_pooled.contiguous()
        dx = torch.empty(B, Hh, Ww, C, dtype=ctx.map_dtype, device=d_pooled.device)
        H.check(H.lib().cvcl_avgpool_bwd(H.cvcl_dtype(ctx.map_dtype), H.ptr(d_pooled, torch.float32), H.ptr(dx), B, Hh * Ww, C,
                                         H.stream_ptr()), "cvcl_avgpool_bwd")
        return None, dx.permute(0, 3, 1, 2)


class _RowsToF32(torch.autograd.Function):
    """bf16 rows of the layer-4 map -> fp32 operand of the 1x1 projection; backward rounds the gradient to the trunk's bf16."""

    @staticmethod
    def forward(ctx, rows):
        rows = rows.contiguous()
        out = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
        H.check(H.lib().cvcl_bf16_to_f32(H.ptr(rows), H.ptr(out), rows.numel(), H.stream_ptr()), "cvcl_bf16_to_f32")
        ctx.dtype = rows.dtype
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_out = d_out.contiguous()
        dx = torch.empty(d_out.shape, dtype=ctx.dtype, device=d_out.device)
        H.check(H.lib().cvcl_f32_to_bf16(H.ptr(d_out, torch.float32), H.ptr(dx), d_out.numel(), H.stream_ptr()), "cvcl_f32_to_bf16")
        return dx


class SpatialResNet(nn.Sequential):
    """embedding_type='spatial' vision model of the reference (multimodal.py:181-185):
    ``nn.Sequential(*list(resnet.children())[:-2], nn.Conv2d(2048, E, 1))`` -- same child indices, hence the same
    state_dict keys (``0.weight`` = conv1 ... ``7.*`` = layer4, ``8.*`` = the 1x1 projection).  The children ARE the
    ResNet's modules (shared parameters); the trunk runs through ``cvcl_resnext50_fwd`` and the projection as an fp32
    GEMM over the per-location rows.  Output: ([B, E, H/32, W/32] view of NHWC rows, layer4 map)."""

    def __init__(self, resnet: ResNet, embedding_dim: int):
        super().__init__(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool, resnet.layer1, resnet.layer2, resnet.layer3,
                         resnet.layer4, nn.Conv2d(2048, embedding_dim, 1))
        object.__setattr__(self, "_resnet", resnet)          # not a registered child: its modules are already children 0..7

    @property
    def compute_dtype(self):
        return self._resnet.compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, dt):
        self._resnet.compute_dtype = dt

    @property
    def trunk_arithmetic(self):
        return self._resnet.trunk_arithmetic

    @trunk_arithmetic.setter
    def trunk_arithmetic(self, a):
        self._resnet.trunk_arithmetic = a

    def train(self, mode: bool = True):
        super().train(mode)
        self._resnet.training = mode
        return self

    def forward(self, x):
        r = self._resnet
        # --finetune_cnn (reference multimodal.py:175-185: autograd through the whole nn.Sequential): r.trunk then returns
        # trunk_train's differentiable layer-4 map, and the gradient of the 1x1 projection flows back into it below
        _pooled, fmap = r.trunk(x)                           # fmap: NCHW view of the NHWC layer-4 map
        for hook in list(self[7]._forward_hooks.values()):   # the reference hooks model[-2] = layer4
            hook(self[7], (fmap,), fmap)
        B, Cc, Hh, Ww = fmap.shape
        rows = fmap.permute(0, 2, 3, 1).reshape(B * Hh * Ww, Cc)
        if rows.dtype != torch.float32:
            rows = _RowsToF32.apply(rows)
        proj = self[8]
        feat = ops.linear_f32(rows, proj.weight.view(proj.out_channels, Cc), proj.bias)       # [B*H*W, E]
        return feat.view(B, Hh, Ww, proj.out_channels).permute(0, 3, 1, 2)


def register_torchvision_alias():
    """Make ``torchvision.models.resnet.{ResNet,Bottleneck}`` resolvable when torchvision is absent, so that the
    reference's Lightning checkpoints (whose ``hyper_parameters`` pickle the whole VisionEncoder, i.e. a torchvision
    ResNet object: multimodal_lit.py:74,139 of the reference) can be unpickled onto these classes."""
    import sys
    import types
    try:
        import torchvision  # noqa: F401  (a real torchvision wins)
        return False
    except Exception:
        pass
    tv = sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    models = sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
    resnet = sys.modules.setdefault("torchvision.models.resnet", types.ModuleType("torchvision.models.resnet"))
    resnet.ResNet, resnet.Bottleneck = ResNet, Bottleneck
    models.resnet, models.resnext50_32x4d = resnet, resnext50_32x4d
    tv.models = models
    return True


def resnext50_32x4d(pretrained: bool = False, **kwargs) -> ResNet:
    if pretrained:
        raise H.CvclError("no network in this environment: ImageNet-pretrained torchvision weights are unavailable")
    return ResNet(**kwargs)
