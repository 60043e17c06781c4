"""CPU: cvcl_trial_scores is declared, bound and exported, refuses every invalid argument with CVCL_EINVAL on dummy pointers without
touching a GPU (the message starts with the entry's name and names the argument), and accepts T = 0 without enqueuing anything."""
import os
import re

import pytest

from conftest import ROOT

FAKE = 0x10000                                          # never dereferenced: validation fails first, and T = 0 launches nothing


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    _hip.load()
    return _hip


def _call(H, query=FAKE, ldq=64, Nq=5, cand=FAKE, ldc=64, Nc=7, D=64, q_idx=FAKE, c_idx=FAKE, T=10, n=4, log_scale=None, logits=None,
          probs=FAKE, pred=FAKE):
    return H.lib().cvcl_trial_scores(query, ldq, Nq, cand, ldc, Nc, D, q_idx, c_idx, T, n, log_scale, logits, probs, pred, None)


def test_declared_bound_exported(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_TRIAL_MAX_CHOICES 16\b", txt) and re.search(r"\bcvcl_trial_scores\s*\(", txt)
    assert "cvcl_trial_scores" in H.SIGNATURES and hasattr(H.lib(), "cvcl_trial_scores")
    assert H.TRIAL_MAX_CHOICES == 16 and len(H.SIGNATURES["cvcl_trial_scores"][1]) == 16
    assert H.lib().cvcl_abi_version() == H.ABI_VERSION and len(H.STRUCTS) == 3           # additive: no version step, no struct
    assert "trials.hip" in os.listdir(os.path.join(ROOT, "multimodal-baby_amd", "csrc"))


@pytest.mark.parametrize("kw,msg", [
    (dict(query=None), b"null pointer (query)"),
    (dict(cand=None), b"null pointer (cand)"),
    (dict(q_idx=None), b"null pointer (q_idx)"),
    (dict(c_idx=None), b"null pointer (c_idx)"),
    (dict(probs=None), b"null pointer (probs)"),
    (dict(pred=None), b"null pointer (pred)"),
    (dict(n=0), b"n 0 outside 1..16"),
    (dict(n=17), b"n 17 outside 1..16"),
    (dict(n=-4), b"n -4 outside 1..16"),
    (dict(D=0), b"D 0 < 1"),
    (dict(D=-8, ldq=-8, ldc=-8), b"D -8 < 1"),
    (dict(ldq=63), b"ldq 63 < D 64"),
    (dict(ldc=0), b"ldc 0 < D 64"),
    (dict(Nq=0), b"Nq 0 < 1"),
    (dict(Nc=-1), b"Nc -1 < 1"),
    (dict(T=-1), b"T -1 < 0"),
    (dict(T=0, query=None), b"null pointer (query)"),      # T = 0 does not switch the validation off
    (dict(T=0, n=17), b"n 17 outside 1..16"),
])
def test_refusals(H, kw, msg):
    rc = _call(H, **kw)
    err = H.lib().cvcl_last_error()
    assert rc == H.EINVAL == -1
    assert err.startswith(b"cvcl_trial_scores: ") and msg in err, err


def test_no_trials_is_a_success(H):
    assert _call(H, T=0) == 0
    assert _call(H, T=0, log_scale=FAKE, logits=FAKE, n=16, D=1, ldq=1, ldc=1, Nq=1, Nc=1) == 0


def test_host_wrapper_refuses_cpu_tensors(H):
    import torch
    from multimodal import trials
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        trials.score_trials(torch.randn(3, 8), torch.randn(4, 8), [0], [[0, 1, 2, 3]])
