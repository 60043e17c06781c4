"""The one way the tools time device work: median [min, max] of repeated device-event windows, the compared sides alternating.

    res = timing.measure({"hip": hip_fn, "eager_torch": torch_fn}, **timing.keywords(args))
    res["hip"] -> {"ms": median, "min_ms", "max_ms", "calls", "samples": [ms per call of each window]}

Per side: ``warmup`` calls, then a probe that sizes a window of back-to-back calls to about ``window_ms`` (calls_for), then ``repeats``
rounds in which every side gets one window in turn.  ``calls=1`` is the per-launch form: every sample is one bracketed launch.
A device that is not there is an error (torch raises in ``window``); nothing here falls back to a host clock."""
import statistics


def window(fn, calls):
    """ms per call of ``calls`` back-to-back calls between two device events; the device is drained before the first event."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def calls_for(fn, window_ms, *, window=window):
    """How many calls fill about ``window_ms``, within 1 .. 20000.  The probe rule: ONE call first; a side whose single call already
    takes ``window_ms`` or longer gets 1 and is not run again; every other side is then probed with one window of FIVE calls (a
    single short launch is mostly event overhead) and gets window_ms over that window's ms per call."""
    if window(fn, 1) >= window_ms:
        return 1
    return max(1, min(20000, int(window_ms / max(window(fn, 5), 1e-6))))


def measure(fns, *, repeats=7, window_ms=200.0, calls=None, warmup=3, window=window):
    """fns: {name: callable}, in order.  ``calls``: None (probe every side), an int, or {name: int} (those sides are not probed).
    -> {name: {"ms", "min_ms", "max_ms", "calls", "samples"}}, ms per call; ``window`` is replaced only by the host test's fake clock."""
    n = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        fixed = calls.get(k) if isinstance(calls, dict) else calls
        n[k] = fixed if fixed is not None else calls_for(fn, window_ms, window=window)
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            samples[k].append(window(fn, n[k]))
    return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": n[k], "samples": v} for k, v in samples.items()}


def add_arguments(ap):
    ap.add_argument("--repeats", type=int, default=7, help="windows per side")
    ap.add_argument("--window-ms", type=float, default=200.0, help="device time one window is sized to")


def keywords(a):
    """the parsed --repeats / --window-ms as measure() keywords"""
    return {"repeats": a.repeats, "window_ms": a.window_ms}


def entry(r, key="ms", scale=1.0, digits=None):
    """One side of measure() under a tool's own key and unit: {key: median, "min_" + key, "max_" + key}, each times ``scale``
    (1e3: us), rounded to ``digits`` when given.  The naming scheme of every tool's output."""
    out = {key: r["ms"] * scale, "min_" + key: r["min_ms"] * scale, "max_" + key: r["max_ms"] * scale}
    return {k: round(v, digits) for k, v in out.items()} if digits is not None else out


def text(r, scale=1.0, spec=".1f"):
    """One side of measure() for the scripts that print lines: 'median [min, max]' times ``scale``."""
    return f"{r['ms'] * scale:{spec}} [{r['min_ms'] * scale:{spec}}, {r['max_ms'] * scale:{spec}}]"


def entries(results, scale=1.0, digits=None):
    """measure()'s whole result flat, for sides named by their output keys: {key, "min_" + key, "max_" + key of every side}."""
    return {k: v for key, r in results.items() for k, v in entry(r, key, scale, digits).items()}
