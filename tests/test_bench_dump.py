"""bench.py --dump-outputs on the host: what the last timed step hands its caller, and the 64 MB cap with a seeded sample."""
import os

import numpy as np
import torch

import bench


def _arrays():
    r = np.random.default_rng(1)
    return {"step.loss": np.asarray(3.5, dtype=np.float64),
            "param.small": r.standard_normal(10).astype(np.float32),
            "param.big": r.standard_normal((40, 25)).astype(np.float32),
            "grad.big": r.standard_normal((20, 25)).astype(np.float32)}


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_write_outputs_whole_arrays_under_the_budget(tmp_path):
    a = _arrays()
    bench.write_outputs(a, str(tmp_path))
    got = _read(tmp_path)
    assert set(got) == set(a)
    for k, v in a.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k


def test_write_outputs_samples_the_large_arrays_the_same_way_every_run(tmp_path):
    a = _arrays()
    budget = 2600                                   # bytes of .npy files: the scalar and the small array whole, the two large sampled
    bench.write_outputs(a, str(tmp_path / "one"), budget=budget)
    bench.write_outputs(_arrays(), str(tmp_path / "two"), budget=budget)
    one, two = _read(tmp_path / "one"), _read(tmp_path / "two")
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")) <= budget
    assert np.array_equal(one["step.loss"], a["step.loss"]) and np.array_equal(one["param.small"], a["param.small"])
    assert one["param.big"].ndim == one["grad.big"].ndim == 1 and 0 < one["param.big"].size == one["grad.big"].size < a["grad.big"].size
    for k in ("param.big", "grad.big"):
        assert np.isin(one[k], a[k].reshape(-1)).all(), k
        assert np.array_equal(one[k], two[k]), k


def test_step_outputs_carries_scalars_trainables_gradients_and_buffers():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    net[0].bias.requires_grad_(False)               # frozen: neither its value nor a gradient is an output
    m = torch.nn.Module()
    m.net = net
    m.alias = net                                   # one module under two names (the lit model holds its encoders so): written once
    loss = m.net(torch.randn(5, 4)).square().mean()
    loss.backward()
    got = bench.step_outputs(m, {"loss": loss, "batch_size": 5, "image_accuracy": torch.tensor(0.25)})
    assert set(got) == {"step.loss", "step.batch_size", "step.image_accuracy", "param.net.0.weight", "grad.net.0.weight",
                        "param.net.1.weight", "grad.net.1.weight", "param.net.1.bias", "grad.net.1.bias",
                        "buffer.net.1.running_mean", "buffer.net.1.running_var"}
    assert got["step.loss"].dtype == np.float64 and float(got["step.loss"]) == float(loss.detach())
    assert got["grad.net.0.weight"].dtype == np.float32 and np.array_equal(got["grad.net.0.weight"], net[0].weight.grad.numpy())
    assert np.array_equal(got["buffer.net.1.running_mean"], net[1].running_mean.numpy())
