"""What an image trunk keeps per process and never pickles: packed weights, workspaces, the trunk stream, deferred work.

``resnext.ResNet``, the DINO ``VisionTransformer``, ``clip_model.VisionTransformer`` and ``clip_model.CLIP`` each hold one
``TrunkRuntime`` as ``self.runtime``.  ``__getstate__`` leaves it out (``strip``) and ``__setstate__`` makes a fresh one, so a
checkpoint -- ``hyper_parameters`` pickles whole encoders -- never carries ctypes arrays, device buffers, streams or events, and an
object unpickled from a reference checkpoint has every slot."""
from __future__ import annotations

import torch

# keys under which earlier versions of the model classes kept this state in their own __dict__: their pickles still carry them
_LEGACY_KEYS = frozenset((
    "_pack_cache", "_ws_cache", "_cache", "_pre_head_callback", "_trunk_stream", "_trunk_out", "_ema_done", "_bn_groups", "_centres",
    "_centres_restored", "_track_centres", "_track_restored", "_centre_sync_pending", "_hip_graphs", "_graphs", "_graph_params"))


def strip(state: dict, *held) -> dict:
    """``state`` (a module's ``__dict__``, or a pickled one) without the runtime attributes ``held`` and without the legacy keys."""
    return {k: v for k, v in state.items() if k not in held and k not in _LEGACY_KEYS}


def fingerprint(params, *extra) -> tuple:
    """"Has a weight changed since I packed it?": ``extra`` + (data_ptr, _version) of every tensor -- an in-place edit advances the
    version, a ``.data`` swap / ``.to()`` / ``load_state_dict(assign=True)`` moves the pointer."""
    return extra + tuple((p.data_ptr(), p._version) for p in params)


class KeyedCache:
    """slot -> (key, value): one value per slot, rebuilt when its key differs from the one it was built under."""

    def __init__(self):
        self.slots = {}

    def get(self, slot, key, build):
        hit = self.slots.get(slot)
        if hit is None or hit[0] != key:
            hit = self.slots[slot] = (key, build())
        return hit[1]


class TrunkRuntime:
    __slots__ = ("defers", "cache", "stream", "buffers", "workspaces", "ema_done", "pre_head_callback", "bn_groups")

    def __init__(self, defers: bool = False):
        self.defers = defers                # the owner's forward runs ``pre_head_callback`` between its trunk and its head
        self.cache = KeyedCache()           # packed weights, resampled position table
        self.stream = None                  # H.TrunkStream, or None: the trunk runs on the caller's stream
        self.buffers = {}                   # persistent device buffers: the output ring per slot, the batch moments per stream
        self.workspaces = {}                # (stream index | "grouped", bytes, device) -> scratch
        self.ema_done = None                # event behind the latest deferred running-statistics update
        self.pre_head_callback = None       # parallel.OverlappedUpdate.flush: the previous step's all-reduce wait + optimizer
        self.bn_groups = None               # ResNet.grouped_bn

    def set_stream(self, stream):
        self.stream, self.ema_done = stream, None
        return stream

    def workspace(self, nbytes: int, device, tag=None):
        """Scratch for the pass on trunk stream ``tag`` (None: the caller's stream), or for the "grouped" walk.  One batch shape
        at a time: a miss drops other shapes' scratch, and a new "grouped" workspace replaces the old one."""
        key = (tag, nbytes, str(device))
        ws = self.workspaces.get(key)
        if ws is None:
            grouped = tag == "grouped"
            for k in [k for k in self.workspaces if (k[0] == "grouped") == grouped and (grouped or k[1:] != key[1:])]:
                del self.workspaces[k]
            ws = self.workspaces[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return ws

    def buffer(self, key, build):
        buf = self.buffers.get(key)
        if buf is None:
            buf = self.buffers[key] = build()
        return buf

    def keep_alive(self) -> list:
        """Everything a captured graph of the owner's forward may reference: it holds these whatever other shapes run later."""
        return list(self.workspaces.values()) + list(self.buffers.values()) + [dict(self.cache.slots)]


def runtime_of(module):
    """``module``'s TrunkRuntime, or None for a module that keeps none."""
    rt = getattr(module, "runtime", None)
    return rt if isinstance(rt, TrunkRuntime) else None
