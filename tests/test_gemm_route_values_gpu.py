"""cvcl_gemm by value over the routing case table (tests/gemm_route_cases.py), through the C ABI only: whatever kernel plan_gemm picks
for a block, C, C_pre, the statistics rows, the accumulators, row_part and a_rowsum hold what the contract in cvcl_hip.h says, as
tests/gemm_route_reference.py evaluates it in float64.

Two input families per case.  random: every element within the reference's derived bound (most elements of a bf16 block: equal);
the column / strip / row sums within 1e-5 of the largest one, against sums of the tensor the kernel itself stored (a statistics-only
block: against its companion run that stores C).  integer: everything equal to the reference, bit for bit.  Every output buffer
carries guard space (one more row, the padding columns, 64 elements behind it), a second call into fresh buffers must give the same
bits, and a case whose buffer is one statistics row short either goes to the next route or is refused with nothing written.
"""
import ctypes as C

import pytest
import torch

from multimodal import _hip as H

import gemm_route_cases as T
import gemm_route_reference as R

PARAMS = [(c, f) for c in T.CASES for f in T.FAMILIES if f == "random" or T.in_integer_family(c)]


_within, _sums_close = R.within, R.sums_close


def _launch(lib, c, family, inputs=None):
    b = T.GpuBlock(lib, c, family=family, guard=True, inputs=inputs)
    rc = lib.cvcl_gemm(c["dt"], C.byref(b.args), H.stream_ptr())
    torch.cuda.synchronize()
    return b, rc


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _guards_intact(b, tag):
    out = {}
    for name in b.outputs():
        vals, guard = b.split_output(name)
        ok = bool((guard == T.CANARY).all()) if guard.dtype == torch.int64 else bool(torch.isnan(guard).all())
        assert ok, f"{tag}: {name}: the call wrote outside what it owns (extra row / padding columns / guard elements)"
        out[name] = vals
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,family", PARAMS, ids=[f"{c['tag']}-{f}" for c, f in PARAMS])
def test_route_values(c, family):
    """Largest err / bound per route on MI355X (256 CUs), random family; the integer family is 0 everywhere.  "sums" is the largest
    of statistics / row_part / a_rowsum against the 1e-5 criterion.  For bf16, "tie / e" is the share of the pre-rounding
    allowance e that an element which rounded the other way shows to be used (its distance to the rounding boundary over e).

        route       C      tie / e  sums        route       C      tie / e  sums
        8w/0        0.990  0.003    0.004       glds/6      0.996  0.518    -
        8w/1        0.991  0.868    0.009       glds/7      0.737  0.000    -
        pro         1.000  0.994    0.007       tiled bf16  0.995  0.961    0.009
        glds/0      0.999  0.005    0.007       tiled fp32  0.105  -        0.009
        glds/1      0.000  -        -           small       0.029  -        -
        glds/2      1.000  0.640    -           split64     0.113  -        0.013
        glds/3      0.961  0.867    -           split3      0.009  -        0.011
        glds/4      0.989  0.138    -           glds/5      0.993  0.792    C_pre 0.349

    bf16 C near 1: an element next to a rounding boundary that falls the other way is off by one ulp against a bound of
    one ulp + e; that is the model, not fragility -- every other element has bound 0 and must match bit for bit (a few hundred
    of millions differ; after GELU about a third, where outputs near 0 have ulps below e).  tie / e is the figure to read: 0.003-0.005
    for plain products (the worst-case (K + 2) 2^-24 accumulation term is ~300 times what the matrix pipe shows), up to 0.99
    where e is made of intermediate roundings (BN operand, tail, residual), which are attained exactly, not estimated.  fp32
    0.03-0.11 is the same worst-case accumulation term against errors that grow like sqrt(K); split3 (0.009) and the small
    kernel under f32_split (0.001) compute more exactly than the documented 2^-16 / six-term allowances they are held to.  The
    1e-5 sums criterion is used at 1 % or less: it is the existing suite's, and the integer family checks the sums exactly.
    The file takes 105 s; the slowest case 5.2 s (pro_plain_below, 131071 x 256 x 128, three float64 products on the CPU)."""
    lib, tag, exact = H.lib(), f"{c['tag']} [{family}]", family == "integer"
    b, rc = _launch(lib, c, family)
    if rc != 0:                                                # a buffer one statistics row short with no further route
        assert c.get("stats") == "short" and "stats_rows" in lib.cvcl_last_error().decode(), f"{tag}: {lib.cvcl_last_error().decode()}"
        for name, vals in _guards_intact(b, tag).items():
            assert bool(torch.isnan(vals).all()), f"{tag}: {name} written by a refused call"
        print(f"{c['tag']:24s} {family:8s} {c['want']:28s} refused: one statistics row short")
        return
    if c["want"].startswith("8w/1"):
        assert lib.cvcl_gemm_ln_supported(C.byref(b.args)) == 1, f"{tag}: the block does not select the 8-wave linear epilogue here"
    if "tile_rows" in c:
        assert lib.cvcl_gemm8w_tile_rows(c["M"], c["N"]) == c["tile_rows"], f"{tag}: the 8-wave tile height the case is there for"
    if T.pad_of(c):
        assert T.stats_rows(lib, c) == T.stats_rows(lib, dict(c, pad=0)), f"{tag}: padded leading dimensions change the statistics rows"
    got = _guards_intact(b, tag)
    ref, bound = R.reference(c, b.ref_inputs(), exact=exact)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    ratios = {}
    for name in ("C", "C_pre"):
        if name in got:
            ratios[name] = _within(f"{tag}: {name}", got[name], ref[name], bound[name])
    stored = got.get("C")
    if c.get("no_C") and not exact:                            # statistics only: against the companion run that stores C
        twin, rc2 = _launch(lib, dict(c, no_C=False), family, inputs=b.inputs)
        assert rc2 == 0, f"{tag}: companion run: {lib.cvcl_last_error().decode()}"
        stored = _guards_intact(twin, tag + " companion")["C"]
    if "stats" in got:
        if c["stats"] == "short":                              # the block went on to a 128 x 128 kernel: one row per grid row, no more
            rows = lib.cvcl_gemm_grid_m(c["dt"], c["M"], c["N"], 0)
            assert bool(torch.isnan(got["stats"][rows:]).all()), f"{tag}: statistics rows past grid_m written"
            got["stats"] = got["stats"][:rows]
        s = R.decode_accumulators(got["stats"]) if c["stats"] == "acc" else got["stats"].double().sum(dim=0)
        ratios["stats"] = (_within(f"{tag}: statistics", s, ref["stats"], torch.zeros_like(s)) if exact else
                           _sums_close(f"{tag}: statistics", s, R.column_sums(stored.double()), (1,)))
    if "row_part" in got:
        ratios["row_part"] = (_within(f"{tag}: row_part", got["row_part"], ref["row_part"], torch.zeros_like(ref["row_part"])) if exact else
                              _sums_close(f"{tag}: row_part", got["row_part"], R.strip_sums(stored.double()), (0, 1)))
    if "a_rowsum" in got:
        ratios["a_rowsum"] = (_within(f"{tag}: a_rowsum", got["a_rowsum"], ref["a_rowsum"], bound["a_rowsum"]) if exact else
                              _sums_close(f"{tag}: a_rowsum", got["a_rowsum"], ref["a_rowsum"], (0,)))
    # a second call into fresh buffers: the same bits, statistics rows and accumulators included
    b2, rc2 = _launch(lib, c, family, inputs=b.inputs)
    assert rc2 == 0
    for name in b.outputs():
        assert torch.equal(_bits(b.t[name]), _bits(b2.t[name])), f"{tag}: {name} differs between two calls on the same inputs"
    differ = int((got["C"].double() != ref["C"]).sum()) if "C" in got else 0
    if differ and "C tie / e" in bound:                        # bf16: a differing element is a rounding that fell the other way
        ratios["C tie/e"] = float(bound["C tie / e"][got["C"].double() != ref["C"]].max())
    print(f"{c['tag']:24s} {family:8s} {c['want']:28s} max err/bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          (f"   ({differ} of {ref['C'].numel()} elements of C differ from the reference)" if "C" in got else ""))
