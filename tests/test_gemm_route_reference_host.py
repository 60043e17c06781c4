"""The float64 reference of the routing case table (tests/gemm_route_reference.py) stands on its own, before a GPU is involved: for
every case with M N K <= 2^27 the contract of cvcl_hip.h, evaluated a second time in plain torch float32 with the bf16 roundings,
stays inside the reference's bound in the random family and equals the reference bit for bit in the integer family, whose
exactness conditions hold.  The larger cases assert the integer family's conditions only, from the reference."""
import pytest
import torch
import torch.nn.functional as F

from multimodal import _hip as H

import gemm_route_cases as T
import gemm_route_reference as R

SMALL = [c for c in T.CASES if c["M"] * c["N"] * c["K"] <= 2 ** 27]
LARGE = [c for c in T.CASES if c["M"] * c["N"] * c["K"] > 2 ** 27 and T.in_integer_family(c)]
PARAMS = [(c, f) for c in SMALL for f in T.FAMILIES if f == "random" or T.in_integer_family(c)]


def contract_f32(c, t):
    """cvcl_gemm's contract in float32 (products and sums as torch takes them), rounding to bf16 where a bf16 block stores or rounds"""
    M, N, K, bf = c["M"], c["N"], c["K"], c["dt"] == T.BF16
    d = {k: v.float() for k, v in t.items() if v.dtype != torch.uint8}

    def rnd(x):
        return x.to(torch.bfloat16).float() if bf else x

    A = d["A"].t() if c.get("a_trans") else d["A"]
    if c.get("gather"):
        ho, wo, hi, wi, s = c["gather"]
        A = A.view(-1, hi, wi, K)[:, 0:ho * s:s, 0:wo * s:s].reshape(-1, K)
    W = R.unpack_f32x3(t["W"], N, K).float() if c["dt"] == T.F32X3 else (d["W"].t() if c.get("w_trans") else d["W"])
    if c.get("prologue"):
        A = A * d["a_scale"] + d["a_shift"]
        A = rnd(F.relu(A) if c["prologue"] == "bn_relu" else A)
    out = {}
    if c.get("a_rowsum"):
        out["a_rowsum"] = A.sum(dim=1)
    acc = A @ W.t()
    if c.get("exp_scale"):
        acc = acc * torch.exp(d["exp_scale"])
    if c.get("tail"):
        p = rnd(acc - d["centre"] if c.get("centre") else acc)
        ident = rnd(d["A2"] @ d["W2"].t() - d["centre2"]) if c.get("ds") else d["R"]
        if "r_scale" in d:
            ident = ident * d["r_scale"] + d["r_shift"]
        v = F.relu(p * d["c_scale"] + d["c_shift"] + ident)
    elif c.get("G"):
        g = d["G"]
        v = rnd(acc) * (0.5 * (1 + torch.erf(g * 2 ** -0.5)) + g * torch.exp(-0.5 * g * g) * 0.3989422804014327)
    else:
        v = acc - d["centre"] if c.get("centre") else acc
        if c.get("ln") == "consumer":
            v = d["ln_stats"][:M, 0:1] * acc + d["ln_stats"][:M, 1:2] * d["ln_colsum"] + d["bias"]
        elif c.get("bias"):
            v = v + d["bias"]
        if c.get("C_pre"):
            v = out["C_pre"] = rnd(v)
        act = c.get("act", T.NONE)
        v = F.relu(v) if act == T.RELU else F.gelu(v) if act == T.GELU else v * torch.sigmoid(1.702 * v) if act == T.QUICK else v
        if c.get("residual"):
            v = rnd(v) + d["R"]
    Cs = rnd(v)
    if not c.get("no_C"):
        out["C"] = Cs
    if c.get("stats"):
        out["stats"] = torch.stack([Cs.sum(dim=0), (Cs * Cs).sum(dim=0)])
    if c.get("ln") == "producer":
        s = Cs.view(M, N // 64, 64)
        out["row_part"] = torch.stack([s.sum(dim=2), (s * s).sum(dim=2)], dim=2)
    return out, Cs.double()


@pytest.mark.parametrize("c,family", PARAMS, ids=[f"{c['tag']}-{f}" for c, f in PARAMS])
def test_reference_against_float32(c, family):
    exact = family == "integer"
    b = T.GpuBlock(H.lib(), c, family=family, device="cpu")
    t = b.ref_inputs()
    ref, bound = R.reference(c, t, exact=exact)                # (exact: raises NotExact where the family's conditions fail)
    got, stored = contract_f32(c, t)                           # (sums are compared with those of the tensor this path stored, as on the GPU)
    assert set(got) == set(ref)
    zero = {k: torch.zeros_like(v) for k, v in ref.items()}
    for name in ("C", "C_pre"):
        if name in got:
            R.within(f"{c['tag']}: {name}", got[name], ref[name], bound[name])
    if "stats" in got:
        if exact:
            R.within(f"{c['tag']}: statistics", got["stats"], ref["stats"], zero["stats"])
        else:
            R.sums_close(f"{c['tag']}: statistics", got["stats"], R.column_sums(stored), (1,))
    if "row_part" in got:
        if exact:
            R.within(f"{c['tag']}: row_part", got["row_part"], ref["row_part"], zero["row_part"])
        else:
            R.sums_close(f"{c['tag']}: row_part", got["row_part"], R.strip_sums(stored), (0, 1))
    if "a_rowsum" in got:
        if exact:
            R.within(f"{c['tag']}: a_rowsum", got["a_rowsum"], ref["a_rowsum"], zero["a_rowsum"])
        else:
            R.sums_close(f"{c['tag']}: a_rowsum", got["a_rowsum"], ref["a_rowsum"], (0,))


@pytest.mark.parametrize("c", LARGE, ids=[c["tag"] for c in LARGE])
def test_integer_family_is_exact_at_large_shapes(c):
    R.reference(c, T.make_inputs(H.lib(), c, "integer"), exact=True)


def test_case_tags_are_unique():
    """a tag seeds its case's inputs and names its tests"""
    assert len({c["tag"] for c in T.CASES}) == len(T.CASES)


def test_rounding_model():
    """bf16_round is nearest-even on the float64 value; tie_distance / round_with_slack cover a value next to a boundary"""
    x = torch.tensor([1.0, 1.00390625, 1.00390626, 1.01171875, 0.998046875, 0.9980468, 0.0, -3.0000001, 257.0, 1e-3], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0078125, 1.015625, 1.0, 0.99609375, 0.0, -3.0, 256.0, float(torch.tensor(1e-3).to(torch.bfloat16))],
                        dtype=torch.float64)
    assert torch.equal(R.bf16_round(x), want)
    d = R.tie_distance(torch.tensor([1.00390625, 1.0, 0.998046875, 1.0000001, 0.0], dtype=torch.float64))
    assert d[0] == 0 and d[1] == 2.0 ** -9 and d[2] == 0 and abs(float(d[3]) - (1e-7 + 2.0 ** -9)) < 1e-12 and d[4] == 0
    # in a random sample, whatever lies further from a boundary than e rounds like every y within e of it
    g = torch.Generator().manual_seed(0)
    v = torch.randn(200000, generator=g, dtype=torch.float64) * 8
    e = torch.full_like(v, 1e-4)
    r, slack = R.round_with_slack(v, e)
    for y in (v + e, v - e):
        assert bool(((R.bf16_round(y) - r).abs() <= slack).all())
    assert 0 < int((slack > 0).sum()) < v.numel() // 10
