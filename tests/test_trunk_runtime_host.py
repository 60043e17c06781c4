"""CPU: the per-process runtime state of the image trunks (multimodal/trunk_runtime.py, resnext.StorageCentres, VisionEncoder's
graph state) -- what is pickled and what is not, the three ``__setstate__`` inputs, the centre state machine, the fingerprint."""
import argparse
import contextlib
import io
import pickle
import threading

import pytest
import torch

import conftest  # noqa: F401  (path setup)
from multimodal import clip_model, resnext, trunk_runtime
from multimodal import vision_transformer_dino_mugs as vits
from multimodal.multimodal import VisionEncoder

# the keys the previous __getstate__ methods wrote, with the values they wrote (ResNet, DINO ViT), and what the classes without a
# __getstate__ carried (clip_model: ``_cache``; VisionEncoder: ``_hip_graphs`` -- ``_graphs`` / ``_graph_params`` were popped)
PARENT_STATE = {
    resnext.ResNet: {"_pack_cache": {}, "_ws_cache": {}, "_pre_head_callback": None, "_trunk_stream": None, "_ema_done": None,
                     "_centres": None, "_track_centres": None, "_centres_restored": None, "_track_restored": None,
                     "_centre_sync_pending": False},
    vits.VisionTransformer: {"_cache": {}, "_pre_head_callback": None},
    clip_model.VisionTransformer: {"_cache": {}},
    clip_model.CLIP: {"_cache": {}},
    VisionEncoder: {"_hip_graphs": True},
}
MODULE_BASE_KEYS = set(torch.nn.Module().__dict__)          # what every pickled nn.Module carries: _parameters, _modules, hooks, ...


def _vision_encoder():
    args = argparse.Namespace(embedding_type="flat", embedding_dim=16, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False,
                              vit_dino=False, finetune_cnn=False)
    with contextlib.redirect_stdout(io.StringIO()):
        return VisionEncoder(args)


def _clip():
    return clip_model.CLIP(embed_dim=32, image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=16, context_length=8,
                           vocab_size=50, transformer_width=64, transformer_layers=1)


BUILDERS = {"resnet": lambda: resnext.ResNet(num_classes=8), "vit": lambda: vits.vit_tiny(), "clip": _clip, "encoder": _vision_encoder}


def _runtimes(m):
    return [sub.runtime for sub in m.modules() if trunk_runtime.runtime_of(sub) is not None]


def _fill(rt):
    """Something unpicklable in every slot."""
    rt.cache.get("w", ("key",), object)
    rt.cache.get("pos_interp", ("key",), threading.Lock)
    rt.stream = object()
    rt.buffers[("out", 0, 2, 2048)] = (object(), threading.Lock())
    rt.buffers[("moments", 0, "cpu")] = threading.Lock()
    rt.workspaces[(None, 64, "cpu")] = object()
    rt.workspaces[("grouped", 64, "cpu")] = object()
    rt.ema_done = threading.Lock()
    rt.pre_head_callback = lambda: None
    rt.bn_groups = 4


def _assert_fresh(rt):
    assert rt.cache.slots == {} and rt.buffers == {} and rt.workspaces == {}
    assert rt.stream is None and rt.ema_done is None and rt.pre_head_callback is None and rt.bn_groups is None
    assert rt.keep_alive() == [{}]


def _assert_fresh_centres(c):
    assert c.frozen is None and c.restored is None and c.tracked is None and c.tracked_restored is None and c.sync_pending is False


def _same_parameters(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_pickle_round_trip_leaves_the_runtime_behind(name):
    torch.manual_seed(0)
    m = BUILDERS[name]()
    rts = _runtimes(m)
    assert len(rts) == {"resnet": 1, "vit": 1, "clip": 2, "encoder": 1}[name]
    for rt in rts:
        _fill(rt)
    resnets = [s for s in m.modules() if isinstance(s, resnext.ResNet)]
    for r in resnets:
        r.centres.frozen = (("key",), torch.ones(53, 2048), threading.Lock())          # (the ready event's place)
        r.centres.restored, r.centres.tracked, r.centres.tracked_restored = torch.ones(1), torch.ones(1), torch.ones(1)
        r.centres.sync_pending = True
    if name == "encoder":
        m.enable_hip_graphs(True)
        m._graphs["shape"] = (object(), threading.Lock())
        m._eval_graphs.params = (0, [threading.Lock()])
    m2 = pickle.loads(pickle.dumps(m))
    assert _same_parameters(m, m2)
    rts2 = _runtimes(m2)
    assert len(rts2) == len(rts) and [rt.defers for rt in rts2] == [rt.defers for rt in rts]
    for rt in rts2:
        _assert_fresh(rt)
    for r in (s for s in m2.modules() if isinstance(s, resnext.ResNet)):
        _assert_fresh_centres(r.centres)
    if name == "encoder":
        assert m2._graphs == {} and m2._eval_graphs.on is None and m2._eval_graphs.params is None
    # the original keeps what it had
    assert rts[0].bn_groups == 4 and (not resnets or resnets[0].centres.sync_pending)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_setstate_takes_the_previous_layout(name):
    """A dict as the previous version's __getstate__ wrote it: a working object, none of its keys left behind."""
    torch.manual_seed(0)
    m = BUILDERS[name]()
    mods = [s for s in m.modules() if type(s) in PARENT_STATE]
    assert mods

    def previous_layout(obj):                           # pickle calls this per object: the tree below ``m`` gets the layout too
        return {**patched[type(obj)](obj), **PARENT_STATE[type(obj)]}
    patched = {}
    try:
        for cls in {type(s) for s in mods}:
            patched[cls] = cls.__getstate__
            cls.__getstate__ = previous_layout
        blob = pickle.dumps(m)
    finally:
        for cls, fn in patched.items():
            cls.__getstate__ = fn
    m2 = pickle.loads(blob)
    assert _same_parameters(m, m2)
    for s in m2.modules():
        if type(s) in PARENT_STATE:
            assert not set(s.__dict__) & set(PARENT_STATE[type(s)]), type(s)
    for rt in _runtimes(m2):
        _assert_fresh(rt)
    if name == "resnet":
        assert m2.export_centres() is None and m2.tracking_centres(torch.device("cpu")) is None and m2.centred_storage() is False
    if name == "encoder":
        assert m2._graphs == {} and m2._eval_graphs.on is None
        assert m2.train(False) is m2 and pickle.loads(pickle.dumps(m2))._graphs == {}
    if name == "vit":
        assert m2.patch_size == 16 and m2.num_heads == 3 and m2.compute_dtype == torch.float32


def test_setstate_takes_the_reference_layout():
    """Objects pickled by the reference's own classes carry nn.Module's base state only (the ViT also what its __init__ sets)."""
    from multimodal import _hip as H
    torch.manual_seed(0)
    src = resnext.ResNet(num_classes=8)
    r = resnext.ResNet.__new__(resnext.ResNet)
    r.__setstate__({k: v for k, v in src.__dict__.items() if k in MODULE_BASE_KEYS})
    assert set(r.__dict__) - MODULE_BASE_KEYS == {"compute_dtype", "trunk_arithmetic", "runtime", "centres"}
    assert r.centred_storage() is False and r.export_centres() is None and r.trunk_dtype() == H.F32
    r.compute_dtype = torch.bfloat16
    assert r.centred_storage() is True and r.trunk_dtype() == H.BF16
    _assert_fresh(r.runtime)
    _assert_fresh_centres(r.centres)
    assert _same_parameters(src, r)

    vsrc = vits.vit_tiny(patch_size=8)
    v = vits.VisionTransformer.__new__(vits.VisionTransformer)
    v.__setstate__({k: val for k, val in vsrc.__dict__.items() if k in MODULE_BASE_KEYS | {"num_features", "embed_dim"}})
    assert v.patch_size == 8 and v.num_heads == 3 and v.compute_dtype == torch.float32
    _assert_fresh(v.runtime)
    assert v.runtime.defers and _same_parameters(vsrc, v)
    v2 = pickle.loads(pickle.dumps(v))                  # ... and its own output
    assert v2.patch_size == 8 and v2.num_heads == 3 and _same_parameters(vsrc, v2)


def test_storage_centres_state_machine():
    """No device, no process group: ``calibrated`` launches nothing itself."""
    c = resnext.StorageCentres()
    x = torch.zeros(1)
    calls = []

    def calibrate():
        calls.append(1)
        return torch.full((53, 2048), float(len(calls)))
    first = c.calibrated(x, "k1", calibrate)
    assert len(calls) == 1 and float(first[0, 0]) == 1.0
    assert c.calibrated(x, "k1", calibrate) is first and len(calls) == 1                 # a hit
    assert float(c.calibrated(x, "k2", calibrate)[0, 0]) == 2.0 and len(calls) == 2      # other weights: a miss
    assert torch.equal(c.export()["frozen"], torch.full((53, 2048), 2.0)) and "tracking" not in c.export()

    saved = torch.arange(53 * 2048, dtype=torch.float32).view(53, 2048)
    c.import_({"frozen": saved, "tracking": None})
    assert c.frozen is None and torch.equal(c.export()["frozen"], saved)                 # restored but unused: still exported
    got = c.calibrated(x, "k3", calibrate)
    assert torch.equal(got, saved) and got is not saved and len(calls) == 2              # restored wins over calibrating
    assert c.restored is None and c.calibrated(x, "k3", calibrate) is got and len(calls) == 2

    c.import_({"frozen": saved})
    c.reset()
    assert c.export() is None and c.sync_pending is False                                # (not distributed: no sync request)
    assert float(c.calibrated(x, "k3", calibrate)[0, 0]) == 3.0 and len(calls) == 3      # reset forgot the cached AND the restored

    cpu = torch.device("cpu")
    t = c.tracking(cpu)
    assert t.shape == (53, 2048) and t.dtype == torch.float32 and not t.any() and c.tracking(cpu) is t
    t.add_(1.0)
    assert torch.equal(c.export()["tracking"], torch.ones(53, 2048))
    c.import_({"frozen": None, "tracking": saved})
    assert c.export() is None                            # (a pending "tracking" restore is adopted by the next tracking() call)
    t2 = c.tracking(cpu)
    assert torch.equal(t2, saved) and c.tracked_restored is None and c.tracking(cpu) is t2
    c.reset()
    assert not c.tracking(cpu).any()
    c.request_sync()
    assert c.sync_pending is True
    c.calibrated(x, "k4", calibrate)                     # no process group: the request stays pending, nobody talks
    assert c.sync_pending is True


def test_resnet_centre_methods_delegate():
    r = resnext.ResNet(num_classes=8)
    saved = torch.ones(53, 2048)
    assert r.export_centres() is None and r.tracking_centres(torch.device("cpu")) is None       # fp32: no centred storage
    r.import_centres({"frozen": saved, "tracking": saved * 2})
    assert torch.equal(r.export_centres()["frozen"], saved)
    r.compute_dtype = torch.bfloat16
    assert torch.equal(r.tracking_centres(torch.device("cpu")), saved * 2)
    r.request_centre_sync()
    assert r.centres.sync_pending is True
    r.recalibrate_centres()
    assert r.export_centres() is None


def test_fingerprint():
    fp = trunk_runtime.fingerprint
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.ones(3))
    f0 = fp([a, b], "bf16", "cuda:0")
    assert f0 == fp(iter([a, b]), "bf16", "cuda:0") and f0[:2] == ("bf16", "cuda:0")
    _ = a.detach() + 1                                   # a no-op for the parameter
    a.requires_grad_(False)
    assert fp([a, b], "bf16", "cuda:0") == f0
    assert fp([a, b], "f32", "cuda:0") != f0 and fp([a], "bf16", "cuda:0") != f0
    with torch.no_grad():
        a.add_(1.0)                                      # in place: the version moves
    f1 = fp([a, b], "bf16", "cuda:0")
    assert f1 != f0
    b.data = torch.ones(3)                               # .data replaced: the pointer moves
    assert fp([a, b], "bf16", "cuda:0") != f1


def test_keyed_cache_and_workspace_eviction():
    c = trunk_runtime.KeyedCache()
    built = []

    def build():
        built.append(1)
        return len(built)
    assert c.get("w", "k", build) == 1 and c.get("w", "k", build) == 1 and c.get("w", "k2", build) == 2 and c.slots["w"][0] == "k2"
    assert c.get("t", "k", build) == 3 and c.get("w", "k2", build) == 2
    rt = trunk_runtime.TrunkRuntime()
    a0, a1 = rt.workspace(64, "cpu", 0), rt.workspace(64, "cpu", 1)
    g = rt.workspace(0, "cpu", "grouped")
    assert rt.workspace(64, "cpu", 0) is a0 and a1 is not a0 and a0.numel() == 64 and g.numel() == 1
    rt.workspace(128, "cpu", 0)                          # another batch shape: the 64-byte scratch of both streams goes, "grouped" stays
    assert set(rt.workspaces) == {(0, 128, "cpu"), ("grouped", 0, "cpu")}
    g2 = rt.workspace(32, "cpu", "grouped")              # a new grouped workspace replaces the old one, plain scratch stays
    assert set(rt.workspaces) == {(0, 128, "cpu"), ("grouped", 32, "cpu")} and rt.workspace(32, "cpu", "grouped") is g2
    rt.workspace(128, "cpu", 1)                          # the same shape on the other stream: nothing goes
    assert len(rt.workspaces) == 3
    out = rt.buffer(("out", 0), lambda: torch.zeros(2))
    assert rt.buffer(("out", 0), lambda: None) is out
    keep = rt.keep_alive()
    assert len(keep) == 5 and any(k is g2 for k in keep) and any(k is out for k in keep) and keep[-1] == {}
