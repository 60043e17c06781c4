"""float64 reference of one cvcl_gemm argument block, with a per-element error bound (tests/gemm_route_cases.py has the blocks).

Written from the contract in include/cvcl_hip.h (the comment block of cvcl_gemm_args), not from the kernels:

    A'  = A | relu?(A * a_scale + a_shift), rows gathered (b, oy, ox) <- (b, oy * stride, ox * stride); K-major with a_trans / w_trans
    acc = A' W^T (* exp(*exp_scale))
    convolution epilogue   C = round(acc - centre)
    Bottleneck tail        C = round(relu(round(acc - centre) * c_scale + c_shift + ident)),
                           ident = R | R * r_scale + r_shift | round(A2 W2^T - centre2) * r_scale + r_shift
    linear epilogue        C = round(round(act(acc + bias)) + R) | round(act(acc + bias));  C_pre = round(acc + bias), C = round(gelu(C_pre))
    GELU backward          C = round(round(acc) * gelu'(G))
    LayerNorm consumer     C = round(act(s0 * acc + s1 * ln_colsum[n] + bias[n])), ln_stats[m] = (s0, s1)
    statistics [2][N] = column (sum, sum of squares) of the stored C; row_part[m][N / 64][2] the same per 64-column strip of a row;
    a_rowsum[m] = sum_k A'[m][k].

"round" is the rounding to bf16 of a bf16 block (nearest even, taken on the float64 value directly); an fp32 block rounds nowhere.
CVCL_F32X3 reads W as the sum of the three bf16 parts cvcl_pack_conv_weight wrote.

The bound.  ``e`` below bounds |kernel's fp32 value - float64 value| BEFORE a rounding, and is built from derivable quantities only:

  accumulation   (K + 2) 2^-24 (|A'| |W|^T): a sum of K products in fp32, in any order, on the matrix pipe or not.  f32_split adds
                 2 * 2^-16 (|A'| |W|^T) (cvcl_hip.h: "products good to ~2^-16 relative").  CVCL_F32X3 (csrc/gemm_split.hip: six part
                 products a0 w0 + a1 w0 + a0 w1 + a0 w2 + a1 w1 + a2 w0 of x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)):
                 |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x|, remainder <= 2^-27 |x|, so the dropped a1 w2 + a2 w1 + a2 w2 and A's remainder
                 are below 2^-24 |a w|, and 6 K part products are summed: (6 K + 3) 2^-24 (|A| |W|^T).
  fp32 epilogue  2^-24 of the magnitude of every operand and result of an fp32 operation (one rounding each; constants below
                 count the operations generously).  expf of exp_scale: 1 ulp of its result.
  rounding       where the contract rounds to bf16, the kernel rounds its own fp32 value y, |y - x| <= e.  If x lies further than e
                 from the nearest rounding boundary (the midpoint of two neighbouring bf16 numbers), round(y) == round(x) and the
                 error becomes ZERO; otherwise y may round to the other neighbour and the error becomes e + ulp(x).  This holds for
                 the stored C as for the intermediates (the prologue's operand, round(acc) before the tail's c_scale, the linear's
                 output before its residual, C_pre).  An
                 intermediate's error is carried on through the absolute factor it meets -- for the operand a second product,
                 slack(A') |W|^T.  No element is excluded anywhere: most elements of a bf16 block must equal the reference bit for
                 bit, the rest may differ by one ulp plus e.  (cvcl_hip.h's "half an ulp" per rounding, <= 2^-8 |ref|, is the
                 distance of a rounded value from the UNROUNDED one; against a rounded reference that allowance would have to be
                 two half ulps, and this model is never wider than that.)
  activations    ReLU is exact and 1-Lipschitz.  GELU (|gelu'| <= 1.13) and QuickGELU (|d/dx| <= 1.10) carry e times that, plus:
                   bf16 GELU   2.6e-5 absolute against the erf form (csrc/cvcl_common.h gelu_bf16out) + 8 2^-24 |x| for its fp32
                               evaluation (the exponent v p carries 2^-24 relative error, v e / (1 + e)^2 |v p| <= 0.45 |v|);
                   fp32 GELU   Abramowitz-Stegun erf 1.5e-7 (cvcl_common.h gelu_erf_fast) enters 0.5 x (1 + erf): 0.75e-7 |x|, plus
                               4 2^-24 (|x| + |gelu|) for the arithmetic around it (1 - erf cancels absolutely, not relatively);
                   QuickGELU   cvcl_common.h: v_exp_f32 / v_rcp_f32 good to ~1 ulp each, result within ~3 fp32 ulp -- for an exact
                               exponent; the exponent -1.702 log2(e) x is itself rounded (2^-24 relative, so e^t is off by
                               |t| 2^-24 <= 2.46 |x| 2^-24 relative): (8 + 4 |x|) 2^-24 |out|;
                   gelu'       0.75e-7 (erf) + 8 2^-24 for the fp32 evaluation of cdf + x pdf (both <= 1.13).

Integer family (gemm_route_cases.make_inputs): ``exact=True`` asserts that every intermediate and stored value is an integer of
magnitude <= 256 (exact in bf16), and per column / row that sum |c| and sum c^2 stay below 2^24 (any fp32 partial sum in any order
is exact).  Then a correct kernel computes the reference bit for bit and every bound is zero.
"""
import math

import torch

import gemm_route_cases as T

EPS = 2.0 ** -24


def bf16_round(x):
    """float64 -> nearest bf16 (ties to even) as float64, without going through float32 (no double rounding)"""
    bits = x.contiguous().view(torch.int64)
    bits = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    return bits.view(torch.float64)


def bf16_ulp(x):
    """spacing of bf16 numbers in the binade of x (8 significant bits); 0 at 0"""
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def tie_distance(x):
    """distance of x to the nearest bf16 rounding boundary (a midpoint of two neighbouring bf16 numbers); 0 at 0"""
    ax = x.abs()
    u = bf16_ulp(ax)
    q = ax / torch.where(u == 0, torch.ones_like(u), u)                  # in [128, 256)
    d = ((q - q.floor()) - 0.5).abs() * u
    low = ax - 128 * u + u / 4                                 # the boundary below the binade's first number: spacing u / 2 there
    return torch.where(ax == 0, torch.zeros_like(ax), torch.minimum(d, low))


def round_with_slack(x, e):
    """(round(x), bound on |round(y) - round(x)| for any |y - x| <= e): zero away from a rounding boundary, e + ulp next to one"""
    near = tie_distance(x) <= e
    return bf16_round(x), torch.where(near, e + bf16_ulp(x), torch.zeros_like(e))


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def unpack_f32x3(packed, n, k):
    """W [N][K] float64 from the bytes cvcl_pack_conv_weight(CVCL_F32X3, CVCL_PACK_DENSE) wrote: [3][N][K] bf16 parts, summed"""
    parts = packed.contiguous().view(torch.bfloat16)
    assert parts.numel() == 3 * n * k, "CVCL_F32X3 dense pack: three bf16 parts of [N][K]"
    return parts.view(3, n, k).double().sum(dim=0)


def worst(err, bound):
    """(largest err / bound, its index); an error where the bound is zero counts as infinite"""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))


def within(what, got, ref, bound):
    """assert that got is finite and within bound of ref everywhere; names the worst element otherwise.  Returns the largest err / bound."""
    assert bool(torch.isfinite(got).all()), f"{what}: not every element was written with a finite value"
    err = (got.double() - ref).abs()
    ratio, at = worst(err, bound)
    assert ratio <= 1.0, (f"{what}: worst element {at}: got {float(got[at])!r}, reference {float(ref[at])!r}, err {float(err[at]):.3e}, "
                          f"bound {float(bound[at]):.3e}, err / bound {ratio:.3f}; {int((err > bound).sum())} of {err.numel()} elements out of bound")
    return ratio


def sums_close(what, got, ref, dims):
    """test_gemm_fused_everything's criterion for sums: within 1e-5 of the largest one (per kind: sums, sums of squares)"""
    scale = ref.abs().amax(dim=dims, keepdim=True) + 1e-30
    return within(what, got, ref, (1e-5 * scale).expand_as(ref))


class NotExact(AssertionError):
    """an integer-family block whose values leave the range in which a correct kernel is exact: the CASE is invalid"""


def column_sums(c):
    """[2][N] float64: column (sum, sum of squares)"""
    return torch.stack([c.sum(dim=0), (c * c).sum(dim=0)])


def strip_sums(c):
    """[M][N / 64][2] float64: (sum, sum of squares) of every 64-column strip of every row"""
    s = c.view(c.shape[0], c.shape[1] // 64, 64)
    return torch.stack([s.sum(dim=2), (s * s).sum(dim=2)], dim=2)


def decode_accumulators(acc):
    """int64 [8][2][N] with 24 fractional bits -> float64 [2][N]: (acc[0] + ... + acc[7]) / 2^24 (the integer sum is exact)"""
    return acc.sum(dim=0).double() / 2.0 ** 24


def reference(c, t, exact=False):
    """c: a case dict; t: name -> input tensor on the CPU in its logical shape (GpuBlock.ref_inputs()).
    Returns (ref, bound): dicts of float64 tensors over the outputs the block asks for -- "C", "C_pre", "stats" [2][N] (of the
    reference's own stored C), "row_part", "a_rowsum"; bound has an entry for C, C_pre and a_rowsum (statistics and row_part are
    compared with sums of the tensor the kernel stored: see the tests), and for a bf16 C also "C tie / e", each element's distance
    to its rounding boundary over e: where a kernel's C differs from the reference, that much of e is shown to be used up.
    exact: assert the integer family's conditions (NotExact)."""
    def mm(x, y):
        return x @ y.T

    M, N, K, dt = c["M"], c["N"], c["K"], c["dt"]
    bf = dt == T.BF16
    d = {k: v.double() for k, v in t.items() if v.dtype != torch.uint8}
    zero = torch.zeros((), dtype=torch.float64)

    def integral(name, x, limit=256.0):
        if exact and not (bool((x == x.round()).all()) and float(x.abs().max()) <= limit):
            raise NotExact(f"{c['tag']}: {name} is not an integer of magnitude <= {limit:g} (max |x| = {float(x.abs().max()):g})")

    def rnd(name, x, e):                                       # a documented rounding: bf16 blocks only
        integral(name, x)
        return round_with_slack(x, e) if bf else (x, e)

    # ---- operands
    A = d["A"].T if c.get("a_trans") else d["A"]
    g = c.get("gather")
    if g:
        ho, wo, hi, wi, s = g
        A = A.view(-1, hi, wi, K)[:, ::s, ::s][:, :ho, :wo].reshape(-1, K)
    assert A.shape == (M, K)
    W = unpack_f32x3(t["W"], N, K) if dt == T.F32X3 else (d["W"].T if c.get("w_trans") else d["W"])
    assert W.shape == (N, K)
    eA = None
    if c.get("prologue"):
        pre = A * d["a_scale"] + d["a_shift"]
        eA = 2 * EPS * ((A * d["a_scale"]).abs() + d["a_shift"].abs())
        if c["prologue"] == "bn_relu":
            eA = torch.where(pre < -eA, torch.zeros_like(eA), eA)
            pre = pre.clamp_min(0.0)
        A, eA = rnd("the prologue's operand", pre, eA)
    A, W = A.contiguous(), W.contiguous()

    # ---- product
    acc = mm(A, W)
    mag = torch.zeros_like(acc) if exact else mm(A.abs(), W.abs())            # (an exact block's bounds are zero: not needed)
    e = ((6 * K + 3) if dt == T.F32X3 else (K + 2)) * EPS * mag
    if c.get("split"):
        e = e + 2 * 2.0 ** -16 * mag
    if eA is not None and not exact:
        e = e + mm(eA.contiguous(), W.abs())
    integral("A'W^T", acc)
    ref, bound = {}, {}
    if c.get("a_rowsum"):
        ref["a_rowsum"], bound["a_rowsum"] = A.sum(dim=1), (K + 1) * EPS * A.abs().sum(dim=1)
        integral("a_rowsum", ref["a_rowsum"], 2.0 ** 24)
        integral("sum_k |A'|", A.abs().sum(dim=1), 2.0 ** 24 - 1)
    if c.get("exp_scale"):
        f = float(torch.exp(d["exp_scale"])[0])
        acc, e = acc * f, e * f + 4 * EPS * (acc * f).abs()

    # ---- epilogue
    if c.get("tail"):
        p = acc - d["centre"] if c.get("centre") else acc
        p, e = rnd("round(A'W^T - centre)", p, e + EPS * p.abs())
        if c.get("ds"):
            A2, W2 = d["A2"].contiguous(), d["W2"].contiguous()
            q = mm(A2, W2) - d["centre2"]
            q, eq = rnd("round(A2 W2^T - centre2)", q, (64 + 2) * EPS * mm(A2.abs(), W2.abs()) + EPS * q.abs())
        elif c.get("residual"):
            q, eq = d["R"], zero
        if "r_scale" in d:
            ident = q * d["r_scale"] + d["r_shift"]
            eq = eq * d["r_scale"].abs() + 2 * EPS * ((q * d["r_scale"]).abs() + d["r_shift"].abs())
        else:
            ident = q
        v = p * d["c_scale"] + d["c_shift"] + ident
        e = e * d["c_scale"].abs() + eq + 4 * EPS * ((p * d["c_scale"]).abs() + d["c_shift"].abs() + ident.abs() + v.abs())
        assert c.get("act") == T.RELU
        v = v.clamp_min(0.0)
    elif c.get("G"):
        p, e = rnd("round(A W^T)", acc, e)
        dg = gelu_grad(d["G"])
        v = p * dg
        e = e * dg.abs() + p.abs() * (0.75e-7 + 8 * EPS) + EPS * v.abs()
    else:
        v = acc
        if c.get("centre"):
            v = v - d["centre"]
            e = e + EPS * v.abs()
        if c.get("ln") == "consumer":
            s0, s1 = d["ln_stats"][:M, 0:1], d["ln_stats"][:M, 1:2]
            v = s0 * acc + s1 * d["ln_colsum"] + d["bias"]
            e = s0.abs() * e + 3 * EPS * ((s0 * acc).abs() + (s1 * d["ln_colsum"]).abs() + d["bias"].abs() + v.abs())
        elif c.get("bias"):
            v = v + d["bias"]
            e = e + EPS * v.abs()
        if c.get("C_pre"):
            v, e = rnd("C_pre", v, e)
            ref["C_pre"], bound["C_pre"] = v, e
        act = c.get("act", T.NONE)
        if act == T.RELU:
            v = v.clamp_min(0.0)
        elif act == T.GELU:
            x, v = v, gelu(v)
            e = 1.13 * e + ((2.6e-5 + 8 * EPS * x.abs()) if bf else (0.75e-7 * x.abs() + 4 * EPS * (x.abs() + v.abs())))
        elif act == T.QUICK:
            x, v = v, quick_gelu(v)
            e = 1.10 * e + (8 + 4 * x.abs()) * EPS * v.abs()
        if c.get("residual"):
            v, e = rnd("the linear's output", v, e)
            v = v + d["R"]
            e = e + EPS * v.abs()
    if bf:
        C, eC = rnd("C", v, e)
        tie = tie_distance(v) / e.clamp_min(1e-300)            # an element that differs shows a pre-rounding error of at least tie * e
    else:
        integral("C", v)
        C, eC = v, e + EPS * v.abs()                           # the fp32 store: half an ulp of fp32
    if exact:
        cs = column_sums(C.abs())
        if float(cs.max()) >= 2.0 ** 24:
            raise NotExact(f"{c['tag']}: a column's sum |c| or sum c^2 reaches 2^24 ({float(cs.max()):g})")
    if not c.get("no_C"):
        ref["C"], bound["C"] = C, eC
        if bf and not exact:
            bound["C tie / e"] = tie
    if c.get("stats"):
        ref["stats"] = column_sums(C)
    if c.get("ln") == "producer":
        ref["row_part"] = strip_sums(C)
    if exact:
        bound = {k: torch.zeros_like(v) for k, v in bound.items()}
    return ref, bound
