"""GPU: the trunks' runtime state with every slot live (multimodal/trunk_runtime.py) -- a model mid-run still pickles, its copy
computes the same bits, and a captured graph holds exactly what ``keep_alive()`` names.  Smallest shapes the trunks take."""
import argparse
import contextlib
import io
import pickle

import pytest
import torch

import conftest  # noqa: F401  (path setup)

pytestmark = pytest.mark.gpu


def _frozen(m, dev):
    for p in m.parameters():
        p.requires_grad_(False)
    m.compute_dtype = torch.bfloat16
    return m.to(dev)


def _three_piped_passes(m, dev, x):
    ts = m.enable_trunk_stream(dev, inputs="ready", n_streams=2)
    with torch.no_grad():
        for _ in range(3):
            m(x)
    ts.join()
    torch.cuda.synchronize(dev)
    return ts


def _copy_computes_the_same(m, dev, x, run):
    blob = pickle.dumps(m)                                       # every runtime slot is live: none of it may reach the pickle
    m2 = pickle.loads(blob).to(dev)
    assert m2.runtime.stream is None and m2.runtime.cache.slots == {} and m2.runtime.buffers == {} and m2.runtime.workspaces == {}
    m.enable_trunk_stream(dev, inputs=None)
    m2.enable_trunk_stream(dev, inputs=None)
    m.eval(), m2.eval()
    with torch.no_grad():
        a, b = run(m, x), run(m2, x)
    torch.cuda.synchronize(dev)
    assert a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b)
    return m2


def test_resnext_pickles_with_every_slot_live(dev):
    from multimodal.resnext import ResNet
    torch.manual_seed(0)
    m = _frozen(ResNet(num_classes=8), dev).train()
    x = torch.randn(2, 3, 64, 64, device=dev)
    _three_piped_passes(m, dev, x)
    rt = m.runtime
    assert sorted(k[0] for k in rt.workspaces) == [0, 1]                                       # scratch per trunk stream
    assert sorted(k[:2] for k in rt.buffers) == [("moments", 0), ("moments", 1), ("out", 0), ("out", 1), ("out", 2)]     # 3 ring slots
    assert rt.ema_done is not None and "pack" in rt.cache.slots
    key, centres, ready = m.centres.frozen
    assert key == rt.cache.slots["pack"][0] and centres.shape == (53, 2048) and ready is not None and float(centres.abs().max()) > 0
    assert int(m.bn1.num_batches_tracked) == 3
    m2 = _copy_computes_the_same(m, dev, x, lambda net, inp: net.trunk(inp)[0])
    assert m2.centres.frozen is None and m2.export_centres() is None and int(m2.bn1.num_batches_tracked) == 3
    assert torch.equal(m.export_centres()["frozen"], centres.cpu())              # (the original keeps its calibration)


def test_vit_pickles_with_every_slot_live(dev):
    from multimodal import vision_transformer_dino_mugs as vits
    torch.manual_seed(0)
    m = _frozen(vits.vit_tiny(patch_size=16), dev).eval()
    x = torch.randn(2, 3, 64, 64, device=dev)                    # T = 17: the resampled position table
    _three_piped_passes(m, dev, x)
    rt = m.runtime
    assert set(rt.cache.slots) == {"w", "pos_interp"} and sorted(k[:2] for k in rt.buffers) == [("out", 0), ("out", 1), ("out", 2)]
    assert rt.stream.n_streams == 2
    _copy_computes_the_same(m, dev, x, lambda net, inp: net(inp))


def test_captured_graph_holds_what_keep_alive_names(dev):
    from multimodal.multimodal import VisionEncoder
    args = argparse.Namespace(embedding_type="flat", embedding_dim=16, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False,
                              vit_dino=False, finetune_cnn=False)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(args)
    ve.to(dev).eval()
    ve.set_compute_dtype(torch.bfloat16)
    rt = ve.model.runtime
    x1 = [torch.randn(1, 3, 64, 64, device=dev) for _ in range(2)]
    x2 = torch.randn(2, 3, 64, 64, device=dev)
    with torch.no_grad():
        eager = [ve(x)[0].clone() for x in x1]
        ve.enable_hip_graphs(True)
        assert torch.equal(ve(x1[0])[0], eager[0]) and len(ve._graphs) == 1
        keep = next(iter(ve._graphs.values()))[4]
        want = rt.keep_alive()
        assert len(keep) == len(want) == 2 and keep[0] is want[0] and keep[0] is next(iter(rt.workspaces.values()))
        assert keep[1].keys() == want[1].keys() == {"pack"} and keep[1]["pack"] is want[1]["pack"]
        ws1, ptr1 = keep[0], keep[0].data_ptr()
        ve(x2)                                                    # another shape: the runtime drops the first shape's scratch ...
        assert len(ve._graphs) == 2 and all(w is not ws1 for w in rt.workspaces.values())
        junk = torch.full((ws1.numel(),), 255, dtype=torch.uint8, device=dev)      # (would land in the freed block)
        assert keep[0].data_ptr() == ptr1 and junk.data_ptr() != ptr1             # ... the first capture still holds it
        assert torch.equal(ve(x1[1])[0], eager[1]) and len(ve._graphs) == 2       # the first graph replayed on new input
        ve.enable_hip_graphs(False)
    torch.cuda.synchronize(dev)
