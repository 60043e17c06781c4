"""GPU: the fp32 text and contrastive-head kernels (csrc/text.hip, csrc/head.hip, cvcl_colsum_f32, cvcl_seq_reverse), one by one through
the C ABI, against float64 on the CPU computed from the same fp32 inputs -- at the shapes the workload has and the toy shapes of the
encoder tests do not: more than one EMB_CHUNK of positions, more than 64 matches of one word, the scalar path of the embedding
backward, grids past their cap, T at the limit of the small attention, arg-max ties across lanes and slices.

Tolerances (the project's own for these kernels, tests/test_head_gpu.py and tests/test_text_train_gpu.py): maxrel < 2e-5 for forward
values, maxrel < 1e-4 for gradients, torch.equal where a kernel only copies, selects or zeroes.  The dropout masks are checked element
by element against a host replica of the counter hash.  Every output starts as NaN.  Each test prints the largest error it saw."""
import math

import numpy as np
import pytest
import torch

from conftest import maxrel

pytestmark = pytest.mark.gpu

NAN = float("nan")
EINVAL = -1
FWD, GRAD = 2e-5, 1e-4
CAP = 8192 * 256                                       # threads of a capped grid-stride launch (cvcl_grid(n, 256, 8192))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    _hip.load()
    return _hip


def run(H, name, *args):
    H.check(getattr(H.lib(), name)(*args, H.stream_ptr()), name)


def nans(dev, *shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def report(what, **errs):
    print(f"[max err] {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items()))


# ---- the dropout hash on the host --------------------------------------------------------------------------------------------------

G0, G1, G2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def hash_uniform(seed, idx):
    """csrc/text.hip hash_uniform in numpy uint64 (wrapping): -> float32 u in [0, 1) for every index of the uint64 array idx."""
    u64 = np.uint64
    with np.errstate(over="ignore"):
        z = np.full(idx.shape, seed, dtype=u64) + idx.astype(u64) * u64(G0)
        z = (z ^ (z >> u64(30))) * u64(G1)
        z = (z ^ (z >> u64(27))) * u64(G2)
        z = z ^ (z >> u64(31))
    return (z >> u64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, idx, p):
    """kept iff u >= float32(p); p == 0 keeps everything (u >= 0)."""
    return torch.from_numpy(hash_uniform(seed, idx) >= np.float32(p))


def seed_with_u(bits24, idx):
    """The seed under which element idx draws u = bits24 * 2^-24 exactly: the hash is a bijection of seed + idx * G0, run backwards."""
    def unshift(y, s):
        x = y
        for _ in range(64 // s + 1):
            x = y ^ (x >> s)
        return x
    z = (bits24 << 40) | 0x5A5A5A5A5A
    z = unshift(z, 31)
    z = (z * pow(G2, -1, 1 << 64)) & M64
    z = unshift(z, 27)
    z = (z * pow(G1, -1, 1 << 64)) & M64
    z = unshift(z, 30)
    return (z - idx * G0) & M64


def test_hash_replica_inverts():
    """The replica against itself: the seed built for (idx, u) gives that u at idx (no GPU work; guards the tie case below)."""
    idx = CAP + 123
    seed = seed_with_u(1 << 23, idx)
    assert float(hash_uniform(seed, np.array([idx], dtype=np.uint64))[0]) == 0.5


# ---- 1. embedding backward ----------------------------------------------------------------------------------------------------------

EMB_CHUNK, EMB_L, EMB_V = 4096, 25, 40
ID_SOS, ID_EOS, ID_64, ID_65, ID_LATE, ID_SCAN, ID_NEVER, ID_FILL0 = 1, 2, 3, 4, 5, 6, 7, 8
_streams = {}


def token_stream(P):
    """-> (tok [P] int64, len [ceil(P / 25)] int64): utterances of 25 positions, <sos> = 1 first, <eos> = 2 at the last valid position,
    pads after it; id 3 exactly 64 times and id 4 exactly 65 times, both in the first chunk of 4096 positions only; id 5 only from
    position 4096 on; id 6 at positions 510..513 (both sides of a 512-position scan edge); id 7 nowhere; the utterance that holds
    position 4096 is full length.  Built once per P and never modified."""
    if P in _streams:
        return _streams[P]
    g = torch.Generator().manual_seed(P)
    B = -(-P // EMB_L)
    ln = torch.randint(2, EMB_L + 1, (B,), generator=g)
    ln[0], ln[1], ln[510 // EMB_L], ln[4096 // EMB_L] = EMB_L, 2, EMB_L, EMB_L
    if B > 8192 // EMB_L:
        ln[8192 // EMB_L] = EMB_L
    tok = torch.randint(ID_FILL0, EMB_V, (B, EMB_L), generator=g)
    pos = torch.arange(EMB_L)[None, :]
    tok[pos >= ln[:, None]] = 0
    tok[:, 0] = ID_SOS
    tok[torch.arange(B), ln - 1] = ID_EOS
    middle = ((pos > 0) & (pos < ln[:, None] - 1)).reshape(-1)
    tok = tok.reshape(-1)
    scan = torch.arange(510, 514)
    assert bool(middle[scan].all()) and bool(middle[4096])
    tok[scan] = ID_SCAN
    middle[scan] = False
    first = torch.nonzero(middle[:EMB_CHUNK]).reshape(-1)
    first = first[torch.randperm(len(first), generator=g)]
    tok[first[:64]] = ID_64
    tok[first[64:129]] = ID_65
    tok[4096] = ID_LATE                                   # (cut off again below when P == 4096)
    late = torch.nonzero(middle[EMB_CHUNK + 1:]).reshape(-1) + EMB_CHUNK + 1
    tok[late[torch.randperm(len(late), generator=g)[:9]]] = ID_LATE
    tok = tok[:P].contiguous()
    count = torch.bincount(tok, minlength=EMB_V)
    assert int(count[ID_64]) == 64 and int(count[ID_65]) == 65 and int(count[ID_NEVER]) == 0
    assert int(count[ID_SOS]) >= min(256, P // EMB_L) > 64 and int(count[ID_EOS]) >= min(256, P // EMB_L)
    assert int(count[ID_LATE]) == (0 if P == EMB_CHUNK else 1 if P == EMB_CHUNK + 1 else 10)
    assert not bool((tok[:EMB_CHUNK] == ID_LATE).any()) and not bool((tok[EMB_CHUNK:] == ID_64).any())
    assert not bool((tok[EMB_CHUNK:] == ID_65).any())
    _streams[P] = (tok, ln)
    return _streams[P]


def embed_ref(src, tok, V):
    """float64 index_add of the source rows [P, E] at the ids inside [0, V), row 0 (padding_idx) zeroed."""
    ok = (tok >= 0) & (tok < V)
    ref = torch.zeros(V, src.shape[1], dtype=torch.float64).index_add_(0, tok[ok], src.double()[ok])
    ref[0] = 0
    return ref


def device_rows(t, dev, misaligned):
    """t on the device; misaligned: as a view one float past a 16-byte boundary (the kernel's scalar path at any E)."""
    if not misaligned:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, device=dev)
    buf[1:] = t.reshape(-1).to(dev)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    return view


def embed_rows_bwd(H, dev, dx, tok, V, misaligned=False):
    """cvcl_embed_rows_bwd twice on NaN-prefilled tables: the two results must be the same bits; -> the table on the CPU."""
    P, E = dx.shape
    dxd, tokd = device_rows(dx, dev, misaligned), tok.to(dev)
    out = []
    for _ in range(2):
        d_table = nans(dev, V, E)
        run(H, "cvcl_embed_rows_bwd", H.ptr(dxd), H.ptr(tokd), H.ptr(d_table), P, E, V)
        torch.cuda.synchronize()
        out.append(d_table.cpu())
    assert torch.equal(out[0], out[1]), "cvcl_embed_rows_bwd does not repeat itself"
    return out[0]


def embed_meanpool_bwd(H, dev, d_ret, tok, ln, V, misaligned=False):
    B, E = d_ret.shape
    dd, tokd, lnd = device_rows(d_ret, dev, misaligned), tok.to(dev), ln.to(dev)
    out = []
    for _ in range(2):
        d_table = nans(dev, V, E)
        run(H, "cvcl_embed_meanpool_bwd", H.ptr(dd), H.ptr(tokd), H.ptr(lnd), H.ptr(d_table), B, EMB_L, E, V)
        torch.cuda.synchronize()
        out.append(d_table.cpu())
    assert torch.equal(out[0], out[1]), "cvcl_embed_meanpool_bwd does not repeat itself"
    return out[0]


def check_table(got, ref, what):
    assert bool(torch.isfinite(got).all()), "a row of d_table was not written"
    assert bool((got[0] == 0).all()) and bool((got[ID_NEVER] == 0).all())
    for v in range(ref.shape[0]):                         # a word that does not occur has a row of exact zeros
        if not bool(ref[v].any()):
            assert bool((got[v] == 0).all()), f"row {v} must be exactly 0"
    per_row = max(maxrel(got[v], ref[v]) for v in range(1, ref.shape[0]) if bool(ref[v].any()))
    e = maxrel(got, ref)
    report(what, table=e, worst_row=per_row)
    assert e < GRAD and per_row < GRAD


EMB_E = [(512, False), (520, False), (6, False), (512, True)]


@pytest.mark.parametrize("E,misaligned", EMB_E)
@pytest.mark.parametrize("P", [4096, 4097, 6400, 9000])
def test_embed_rows_bwd_vs_float64(H, dev, P, E, misaligned):
    """cvcl_embed_rows_bwd over 1, 1 + one position, 2 and 3 chunks of positions; E = 512 (one pass), 520 (two passes of EMB_PASS), 6 and
    a misaligned dx (the scalar path).  <sos> / <eos> have >= 163 matches in the first chunk (three deals of 64 to the groups), ids 3 /
    4 sit at 64 / 65 matches (the edge of one deal), id 5 occurs only behind the first chunk, id 6 straddles a scan edge.  Each row is
    held to 1e-4 of its own largest entry as well as the table to 1e-4 of its largest: a dropped chunk or deal of one word shows."""
    tok, _ = token_stream(P)
    dx = torch.randn(P, E, generator=torch.Generator().manual_seed(P + E))
    got = embed_rows_bwd(H, dev, dx, tok, EMB_V, misaligned)
    check_table(got, embed_ref(dx, tok, EMB_V), f"embed_rows_bwd P {P} E {E} misaligned {misaligned}")


@pytest.mark.parametrize("E,misaligned", EMB_E)
@pytest.mark.parametrize("P", [6400, 9000])
def test_embed_meanpool_bwd_vs_float64(H, dev, P, E, misaligned):
    """cvcl_embed_meanpool_bwd at B = 256 and 360 utterances of L = 25: the full-length utterance 163 holds positions 4075..4099, on both
    sides of the first chunk edge, and utterance 327 those around 8192.  Reference: d_ret[b] / len[b] in float64 at every position."""
    tok, ln = token_stream(P)
    B = P // EMB_L
    d_ret = torch.randn(B, E, generator=torch.Generator().manual_seed(P + E + 1))
    src = (d_ret.double() / ln[:, None].double()).repeat_interleave(EMB_L, 0)
    got = embed_meanpool_bwd(H, dev, d_ret, tok, ln, EMB_V, misaligned)
    check_table(got, embed_ref(src, tok, EMB_V), f"embed_meanpool_bwd P {P} E {E} misaligned {misaligned}")


@pytest.mark.parametrize("E", [512, 6])
def test_embed_bwd_out_of_range_ids_reach_no_row(H, dev, E):
    """Ids -1, V, 5 + 2^32 (its low 32 bits are the in-range id 5), 3 + 2^33 and -1 - 2^32 at filler positions: the result equals the
    float64 reference without those positions, and is bit for bit what the kernel gives with pads in their place (a pad reaches no
    row either and the order of the other matches is the same).  Both forms of the kernel."""
    P = 6400
    tok, ln = token_stream(P)
    filler = torch.nonzero(tok >= ID_FILL0).reshape(-1)
    bad_ids = [-1, EMB_V, 5 + 2 ** 32, 3 + 2 ** 33, -1 - 2 ** 32, EMB_V + 2 ** 40]
    at = filler[torch.randperm(len(filler), generator=torch.Generator().manual_seed(E))[:10 * len(bad_ids)]]
    assert bool((at < EMB_CHUNK).any()) and bool((at >= EMB_CHUNK).any())
    bad, padded = tok.clone(), tok.clone()
    bad[at] = torch.tensor(bad_ids * 10)
    padded[at] = 0
    dx = torch.randn(P, E, generator=torch.Generator().manual_seed(E + 7))
    got = embed_rows_bwd(H, dev, dx, bad, EMB_V)
    check_table(got, embed_ref(dx, bad, EMB_V), f"embed_rows_bwd out-of-range ids E {E}")
    assert torch.equal(got, embed_rows_bwd(H, dev, dx, padded, EMB_V))
    d_ret = torch.randn(P // EMB_L, E, generator=torch.Generator().manual_seed(E + 8))
    src = (d_ret.double() / ln[:, None].double()).repeat_interleave(EMB_L, 0)
    got = embed_meanpool_bwd(H, dev, d_ret, bad, ln, EMB_V)
    check_table(got, embed_ref(src, bad, EMB_V), f"embed_meanpool_bwd out-of-range ids E {E}")
    assert torch.equal(got, embed_meanpool_bwd(H, dev, d_ret, padded, ln, EMB_V))


# ---- 2. dropout ---------------------------------------------------------------------------------------------------------------------

DROP_N = (1 << 21) + 300                                  # past the 8192 x 256 threads of the capped grid: a second trip of the loop
TIE_IDX = CAP + 123                                       # an element of that second trip
DROP_SEEDS = [2 ** 62 - 1, 12345, seed_with_u(1 << 23, TIE_IDX)]   # under the third, element TIE_IDX draws u = 0.5 exactly


def big_input(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (1 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()      # 1 <= |x| < 2
    return x, torch.randn(n, generator=g)


def dropout(H, dev, x, r, p, seed, period=0, inner=0):
    y = nans(dev, x.numel())
    xd, rd = x.to(dev), r.to(dev) if r is not None else None
    run(H, "cvcl_dropout", H.ptr(xd), H.ptr(rd), H.ptr(y), x.numel(), p, seed, period, inner)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("seed", DROP_SEEDS)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_mask_is_the_hash_of_seed_and_index(H, dev, p, seed):
    """The zero pattern of y (|x| >= 1, no residual) is the replica's mask, element by element; a kept element is x / (1 - p) to 2^-23
    relative (p as the float32 the kernel receives); p == 0 returns x.  With the third seed and p = 0.5 one element draws u == p
    exactly: it is kept (u >= p).  With a residual: y = dropout(x) + r against float64 with the replica's mask."""
    x, r = big_input(DROP_N, 5)
    keep = keep_mask(seed, np.arange(DROP_N, dtype=np.uint64), p)
    if p == 0.5 and seed == DROP_SEEDS[2]:
        u = hash_uniform(seed, np.array([TIE_IDX], dtype=np.uint64))
        assert float(u[0]) == 0.5 and bool(keep[TIE_IDX])
    if p == 0.0:
        assert bool(keep.all())
    y = dropout(H, dev, x, None, p, seed)
    wrong = int(((y != 0) != keep).sum())
    assert wrong == 0, f"{wrong} elements kept / dropped against the hash (first at {int(torch.nonzero((y != 0) != keep)[0])})"
    p32 = float(np.float32(p))
    ref = x.double() / (1.0 - p32)
    e_keep = float(((y.double() - ref).abs() / ref.abs())[keep].max())
    assert e_keep <= 2.0 ** -23
    if p == 0.0:
        assert torch.equal(y, x)
    yr = dropout(H, dev, x, r, p, seed)
    e_res = maxrel(yr, torch.where(keep, ref, torch.zeros_like(ref)) + r.double())
    report(f"dropout p {p} seed {seed}", kept_rel=e_keep, with_residual=e_res)
    assert e_res < FWD
    if p == 0.0:
        assert torch.equal(yr, x + r)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_locked_mask_is_shared_over_the_period(H, dev, p):
    """LockedDropout's form: x [B = 7][L = 25][E = 512], period L, inner E: the mask of element (b, l, e) is the hash at b E + e."""
    B, L, E, seed = 7, 25, 512, 2 ** 62 - 1
    x, _ = big_input(B * L * E, 6)
    keep = keep_mask(seed, np.arange(B * E, dtype=np.uint64), p).reshape(B, 1, E).expand(B, L, E)
    assert 0 < int(keep.sum()) < keep.numel()
    y = dropout(H, dev, x, None, p, seed, L, E).reshape(B, L, E)
    assert torch.equal(y != 0, keep)
    ref = x.double().reshape(B, L, E) / (1.0 - float(np.float32(p)))
    e = float(((y.double() - ref).abs() / ref.abs())[keep].max())
    report(f"dropout locked p {p}", kept_rel=e)
    assert e <= 2.0 ** -23


# ---- 3. small attention -------------------------------------------------------------------------------------------------------------

ATT_SHAPES = [(3, 25, 8, 64, [1, 25, 13]), (2, 32, 8, 64, [32, 1]), (4, 1, 2, 8, [1, 1, 1, 1]), (3, 7, 3, 5, [1, 7, 4])]
ATT_SEED = 2 ** 62 - 1


def attn_inputs(B, T, heads, hd, lens):
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = torch.randn(B, T, 3, heads, hd, generator=g)
    d_out = torch.randn(B, T, heads * hd, generator=g)
    tok = torch.randint(1, 50, (B, T), generator=g)
    tok[torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]] = 0
    return qkv, tok, d_out


def attn_ref(qkv, tok, d_out, scale, p, seed):
    """float64 masked softmax attention with the replica's dropout mask on P, and its autograd: -> (out [B, T, D], d_qkv)."""
    B, T, _, heads, hd = qkv.shape
    x = qkv.double().requires_grad_(True)
    s = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) * scale
    s = s.masked_fill((tok == 0)[:, None, None, :], -math.inf)
    P = torch.softmax(s, -1)
    if p > 0:
        keep = keep_mask(seed, np.arange(B * heads * T * T, dtype=np.uint64), p).reshape(B, heads, T, T)
        P = P * keep / (1.0 - float(np.float32(p)))
    out = torch.einsum("bhij,bjhd->bihd", P, x[:, :, 2]).reshape(B, T, heads * hd)
    out.backward(d_out.double())
    return out.detach(), x.grad


def attn_call(H, dev, qkv, tok, d_out, scale, p, seed, fwd=True, bwd=True):
    B, T, _, heads, hd = qkv.shape
    out, d_qkv = nans(dev, B, T, heads * hd), nans(dev, *qkv.shape)
    qkvd, tokd, d_outd = qkv.to(dev), tok.to(dev), d_out.to(dev)
    run(H, "cvcl_attention_small", H.ptr(qkvd), H.ptr(tokd), H.ptr(d_outd) if bwd else None, H.ptr(out) if fwd else None,
        H.ptr(d_qkv) if bwd else None, B, T, heads, hd, scale, p, seed)
    torch.cuda.synchronize()
    return out.cpu(), d_qkv.cpu()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,heads,hd,lens", ATT_SHAPES)
def test_attention_small_vs_float64(H, dev, B, T, heads, hd, lens, p):
    """cvcl_attention_small at the workload's T = 25 x hd = 64, the limit T = 32, one token, and odd T / heads / hd; utterance lengths 1
    and T among them.  Forward at 2e-5, d_qkv at 1e-4 against float64 autograd (dropout mask: the replica at
    ((b heads + h) T + i) T + j, scaled by 1 / (1 - p)); dk / dv of a masked key are exactly 0; the forward-only and the backward-only
    call (as csrc/text.hip's callers make them) give the bits of the combined call and leave the other output alone."""
    qkv, tok, d_out = attn_inputs(B, T, heads, hd, lens)
    scale = float(np.float32(hd ** -0.5))
    out_ref, dq_ref = attn_ref(qkv, tok, d_out, scale, p, ATT_SEED)
    out, d_qkv = attn_call(H, dev, qkv, tok, d_out, scale, p, ATT_SEED)
    e_out, e_dq = maxrel(out, out_ref), maxrel(d_qkv, dq_ref)
    report(f"attention_small B {B} T {T} heads {heads} hd {hd} p {p}", out=e_out, d_qkv=e_dq)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_qkv).all())
    assert e_out < FWD and e_dq < GRAD
    masked = tok == 0
    assert bool((d_qkv[:, :, 1][masked] == 0).all()) and bool((d_qkv[:, :, 2][masked] == 0).all())
    out_f, dq_f = attn_call(H, dev, qkv, tok, d_out, scale, p, ATT_SEED, bwd=False)
    assert torch.equal(out_f, out) and bool(torch.isnan(dq_f).all())
    out_b, dq_b = attn_call(H, dev, qkv, tok, d_out, scale, p, ATT_SEED, fwd=False)
    assert torch.equal(dq_b, d_qkv) and bool(torch.isnan(out_b).all())


def test_attention_small_refuses_T_33(H, dev):
    B, T, heads, hd = 2, 33, 2, 8
    qkv, tok, d_out = attn_inputs(B, T, heads, hd, [33, 5])
    out, d_qkv = nans(dev, B, T, heads * hd), nans(dev, *qkv.shape)
    qkvd, tokd, d_outd = qkv.to(dev), tok.to(dev), d_out.to(dev)
    rc = H.lib().cvcl_attention_small(H.ptr(qkvd), H.ptr(tokd), H.ptr(d_outd), H.ptr(out), H.ptr(d_qkv), B, T, heads, hd, hd ** -0.5, 0.1,
                                      1, H.stream_ptr())
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(d_qkv).all())


# ---- 4. LayerNorm backward, column sums, ReLU backward ----------------------------------------------------------------------------

def colsum(H, dev, a):
    M, N = a.shape
    out, ad = nans(dev, N), a.to(dev)
    run(H, "cvcl_colsum_f32", H.ptr(ad), H.ptr(out), M, N)
    torch.cuda.synchronize()
    return out.cpu()


def ln_bwd_case(H, dev, rows, D, mean):
    g = torch.Generator().manual_seed(rows * 1000 + D)
    x = torch.randn(rows, D, generator=g) + mean
    dy = torch.randn(rows, D, generator=g) + 0.3
    gamma = torch.rand(D, generator=g) + 0.5
    eps = 1e-5
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), torch.zeros(D, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(x64, (D,), g64, b64, eps).backward(dy.double())
    xd, dyd, gammad = x.to(dev), dy.to(dev), gamma.to(dev)
    dx, dyxh = nans(dev, rows, D), nans(dev, rows, D)
    run(H, "cvcl_layernorm_bwd", H.ptr(xd), H.ptr(gammad), H.ptr(dyd), eps, H.ptr(dx), H.ptr(dyxh), rows, D)
    dg, db = colsum(H, dev, dyxh), colsum(H, dev, dyd)             # as text_train.py forms dgamma / dbeta
    e = dict(dx=maxrel(dx, x64.grad), dgamma=maxrel(dg, g64.grad), dbeta=maxrel(db, b64.grad))
    report(f"layernorm_bwd rows {rows} D {D} mean {mean}", **e)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dyxh).all())
    assert max(e.values()) < GRAD


@pytest.mark.parametrize("D", [7, 32, 512, 520])
@pytest.mark.parametrize("rows", [1, 5, 6400])
def test_layernorm_bwd_vs_float64(H, dev, rows, D):
    """cvcl_layernorm_bwd (one wave per row, four rows per workgroup): 1 and 5 rows leave waves of the last workgroup idle, 6400 is the
    workload's B L; D = 7 and 32 leave lanes idle, 520 gives 8 lanes a ninth element.  dx, and dgamma / dbeta through cvcl_colsum_f32
    as the text encoder's backward obtains them, against float64 autograd of F.layer_norm; gamma in [0.5, 1.5), dy of mean 0.3."""
    ln_bwd_case(H, dev, rows, D, 0.0)


def test_layernorm_bwd_rows_of_mean_10_unit_spread(H, dev):
    """Row means ~ 10 with unit spread: x - mean cancels a decimal digit; an E[x^2] - mean^2 variance would lose seven."""
    ln_bwd_case(H, dev, 300, 512, 10.0)


@pytest.mark.parametrize("N", [1, 15, 17, 12800])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 6400])
def test_colsum_f32_vs_float64(H, dev, M, N):
    """cvcl_colsum_f32: 16 columns x 64 row slices per workgroup; M = 1 / 63 leave slices empty, 64 / 65 put one / two rows in slice 0;
    N = 15 / 17 end inside a workgroup's columns; 6400 x 12800 is more rows than the text encoder's d_pos sum over [B][L E]."""
    a = torch.randn(M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(M * 7 + N)) + 0.5
    ref = a.cpu().double().sum(0)
    e = maxrel(colsum(H, dev, a), ref)
    report(f"colsum_f32 M {M} N {N}", colsum=e)
    assert e < FWD


def test_relu_bwd_is_exact(H, dev):
    """dx = dy where y > 0, else 0: +0, -0 and negative y give exact zeros; n is past the capped grid."""
    n = DROP_N
    g = torch.Generator().manual_seed(11)
    y = torch.randn(n, generator=g)
    kind = torch.randint(0, 4, (n,), generator=g)
    y[kind == 0] = 0.0
    y[kind == 1] = -0.0
    y[-1], y[-2], y[CAP], y[CAP + 1] = 1.0, -0.0, 2.0, 0.0
    dy = torch.randn(n, generator=g)
    dx, yd, dyd = nans(dev, n), y.to(dev), dy.to(dev)
    run(H, "cvcl_relu_bwd", H.ptr(yd), H.ptr(dyd), H.ptr(dx), n)
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), torch.where(y > 0, dy, torch.zeros_like(dy)))


# ---- 5. InfoNCE, entropies, token cross-entropy -------------------------------------------------------------------------------------

def infonce_logits(N):
    """logits [N, N] = 100 img txt^T of unit rows (the diagonal of a matched pair is 100, the rest within about +-60), with exact ties:
    for (a, b) in row_pairs, txt[a] = txt[b] = img[a]: row a has its maximum at columns a and b; for (a, b) in col_pairs,
    img[a] = img[b] = txt[a]: column a has its maximum at rows a and b.  The first of each pair is the diagonal: under the
    first-maximum rule the row / column counts as a hit, under a last-maximum rule it would not."""
    g = torch.Generator().manual_seed(N)
    img = torch.nn.functional.normalize(torch.randn(N, 32, generator=g), dim=1)
    txt = torch.nn.functional.normalize(0.5 * img + torch.randn(N, 32, generator=g), dim=1)
    row_pairs = [(0, 64), (10, 13)] + ([(40, 104), (70, 77)] if N > 104 else [])       # same lane (j, j + 64) / across lanes
    col_pairs = [(5, 21), (30, 33)] + ([(90, 106), (110, 125)] if N > 125 else [])      # same slice (r, r + 16) / across slices
    for a, b in col_pairs:
        img[a] = img[b] = txt[a]
    for a, b in row_pairs:
        txt[a] = txt[b] = img[a]
    logits = ((img.double() @ txt.double().t()) * 100).float()
    for a, b in row_pairs:
        logits[:, b] = logits[:, a]
    for a, b in col_pairs:
        logits[b, :] = logits[a, :]
    for a, b in row_pairs:
        assert float(logits[a, a]) == float(logits[a, b]) == float(logits[a].max()) and int((logits[a] == logits[a].max()).sum()) == 2
    for a, b in col_pairs:
        assert float(logits[a, a]) == float(logits[b, a]) == float(logits[:, a].max())
        assert int((logits[:, a] == logits[:, a].max()).sum()) == 2
    return logits.contiguous(), row_pairs, col_pairs


def entropy64(x, dim):
    lp = torch.log_softmax(x, dim)
    return -(lp.exp() * lp).sum(dim)


@pytest.mark.parametrize("N", [65, 130])
def test_infonce_fwd_bwd_vs_float64_with_ties(H, dev, N):
    """cvcl_infonce_fwd / _bwd on logits of about +-100 with arg-max ties inside one lane's / one slice's sequence (j and j + 64, r and
    r + 16) and across lanes / slices.  Accuracies: torch.argmax's first maximum on the same fp32 matrix, to 1e-6 (a count / N);
    row_lse / col_lse at 2e-5; the loss and the two entropies each to 2e-5 of its own value; d_logits at d_loss = 0.37 against
    float64 autograd at 1e-4."""
    logits, row_pairs, col_pairs = infonce_logits(N)
    ar = torch.arange(N)
    acc_i, acc_t = (logits.argmax(1) == ar).double().mean(), (logits.argmax(0) == ar).double().mean()
    last_i = ((N - 1 - logits.flip(1).argmax(1)) == ar).double().mean()
    last_t = ((N - 1 - logits.flip(0).argmax(0)) == ar).double().mean()
    assert float(acc_i - last_i) * N >= len(row_pairs) - 0.5 and float(acc_t - last_t) * N >= len(col_pairs) - 0.5
    x = logits.double().requires_grad_(True)
    loss = (torch.nn.functional.cross_entropy(x, ar) + torch.nn.functional.cross_entropy(x.t(), ar)) / 2
    d_loss = 0.37
    (loss * d_loss).backward()
    ref5 = torch.stack([loss.detach(), acc_i, acc_t, entropy64(x.detach(), 1).mean(), entropy64(x.detach(), 0).mean()])
    xd = logits.to(dev)
    scal, row_lse, col_lse = nans(dev, 5), nans(dev, N), nans(dev, N)
    nb = H.lib().cvcl_infonce_workspace_bytes(N)
    ws = nans(dev, nb // 4)
    run(H, "cvcl_infonce_fwd", H.ptr(xd), N, H.ptr(scal), H.ptr(row_lse), H.ptr(col_lse), H.ptr(ws), nb)
    d_logits, d_lossd = nans(dev, N, N), torch.tensor([d_loss], device=dev)
    run(H, "cvcl_infonce_bwd", H.ptr(xd), H.ptr(row_lse), H.ptr(col_lse), H.ptr(d_lossd), H.ptr(d_logits), N)
    torch.cuda.synchronize()
    scal = scal.cpu().double()
    err5 = (scal - ref5).abs()
    e = dict(row_lse=maxrel(row_lse, torch.logsumexp(x.detach(), 1)), col_lse=maxrel(col_lse, torch.logsumexp(x.detach(), 0)),
             loss=float(err5[0]), img_acc=float(err5[1]), txt_acc=float(err5[2]), img_entropy=float(err5[3]),
             txt_entropy=float(err5[4]), d_logits=maxrel(d_logits, x.grad))
    report(f"infonce N {N} (scalars: absolute; reference {[round(float(v), 4) for v in ref5]})", **e)
    assert e["img_acc"] < 1e-6 and e["txt_acc"] < 1e-6
    assert e["row_lse"] < FWD and e["col_lse"] < FWD
    for k in (0, 3, 4):
        assert float(err5[k]) < FWD * abs(float(ref5[k]))
    assert e["d_logits"] < GRAD


@pytest.mark.parametrize("R,N", [(5, 1), (3, 65), (6400, 2350)])
def test_row_entropy_vs_float64(H, dev, R, N):
    """cvcl_row_entropy: one column (entropy exactly 0), one more column than lanes, the language model's B L x vocabulary."""
    x = torch.randn(R, N, device=dev, generator=torch.Generator(device=dev).manual_seed(R + N)) * 3
    out = nans(dev, R)
    run(H, "cvcl_row_entropy", H.ptr(x), H.ptr(out), R, N)
    torch.cuda.synchronize()
    e = maxrel(out, entropy64(x.cpu().double(), 1))
    report(f"row_entropy R {R} N {N}", entropy=e)
    if N == 1:
        assert bool((out == 0).all())
    assert e < FWD


def token_ce_case(H, dev, logits, labels, ignore):
    R, V = logits.shape
    g = torch.Generator().manual_seed(R + V)
    d_loss = torch.randn(R, generator=g)
    live = (labels != ignore) & (labels >= 0) & (labels < V)
    x = logits.double().requires_grad_(True)
    lp = torch.log_softmax(x, 1)
    loss_ref = torch.where(live, -lp.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0], torch.zeros(R, dtype=torch.float64))
    (loss_ref * d_loss.double()).sum().backward()
    xd, labd, d_lossd = logits.to(dev), labels.to(dev), d_loss.to(dev)
    loss, lse, d_logits = nans(dev, R), nans(dev, R), nans(dev, R, V)
    run(H, "cvcl_token_ce_fwd", H.ptr(xd), H.ptr(labd), H.ptr(loss), H.ptr(lse), R, V, ignore)
    run(H, "cvcl_token_ce_bwd", H.ptr(xd), H.ptr(labd), H.ptr(lse), H.ptr(d_lossd), H.ptr(d_logits), R, V, ignore)
    torch.cuda.synchronize()
    loss, lse, d_logits = loss.cpu(), lse.cpu(), d_logits.cpu()
    assert bool((loss[~live] == 0).all()) and bool((d_logits[~live] == 0).all())
    e_lse = maxrel(lse, torch.logsumexp(x.detach(), 1))
    e_loss = maxrel(loss, loss_ref.detach()) if bool(live.any()) else 0.0
    e_d = maxrel(d_logits, x.grad) if bool(live.any()) else 0.0
    assert e_lse < FWD and e_loss < FWD and e_d < GRAD
    return e_lse, e_loss, e_d


@pytest.mark.parametrize("V", [17, 255, 257, 2350])
@pytest.mark.parametrize("R", [1, 300])
def test_token_ce_fwd_bwd_vs_float64(H, dev, R, V):
    """cvcl_token_ce_fwd / _bwd: V below, one under, one over the 256 threads of a row's workgroup, and the vocabulary's size.  Labels
    with the ignore index (0), -1 and V: loss 0 and a zero gradient row, exactly.  The one-row case runs once with each such label and
    once with a live one.  Random d_loss; float64 log_softmax."""
    g = torch.Generator().manual_seed(R * 31 + V)
    logits = torch.randn(R, V, generator=g) * 5
    if R == 1:
        errs = [token_ce_case(H, dev, logits, torch.tensor([lab]), 0) for lab in (V - 1, 0, -1, V)]
    else:
        labels = torch.randint(1, V, (R,), generator=g)
        labels[::7], labels[3::11], labels[5::13] = 0, -1, V
        labels[-1] = V - 1
        errs = [token_ce_case(H, dev, logits, labels, 0)]
    report(f"token_ce R {R} V {V}", lse=max(e[0] for e in errs), loss=max(e[1] for e in errs), d_logits=max(e[2] for e in errs))


def test_lm_loss_summaries_vs_float64(H, dev):
    """cvcl_lm_loss_summaries at R = 6400: the three means of multimodal_lit.py:284-300 -- sum(loss) / #non-pad, then the sums over the
    tokens that are not <sos>, and neither <sos> nor <eos>, over their counts (the loss of a pad is 0, as cvcl_token_ce_fwd leaves
    it) -- the counts exactly, and the backward against float64 autograd of those three means."""
    R, pad, sos, eos = 6400, 0, 1, 2
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 12, (R,), generator=g)
    m0 = labels != pad
    m1, m2 = m0 & (labels != sos), m0 & (labels != sos) & (labels != eos)
    assert 0 < int(m2.sum()) < int(m1.sum()) < int(m0.sum()) < R
    loss = (torch.rand(R, generator=g) * 8) * m0
    d_means = torch.tensor([0.7, -1.3, 2.1])
    x = loss.double().requires_grad_(True)
    means_ref = torch.stack([x.sum() / m0.sum(), (x * m1).sum() / m1.sum(), (x * m2).sum() / m2.sum()])
    (means_ref * d_means.double()).sum().backward()
    labd, lossd, d_meansd = labels.to(dev), loss.to(dev), d_means.to(dev)
    means, counts, d_loss = nans(dev, 3), nans(dev, 3), nans(dev, R)
    run(H, "cvcl_lm_loss_summaries", H.ptr(lossd), H.ptr(labd), None, H.ptr(means), H.ptr(counts), None, R, pad, sos, eos)
    run(H, "cvcl_lm_loss_summaries", None, H.ptr(labd), H.ptr(d_meansd), None, H.ptr(counts), H.ptr(d_loss), R, pad, sos, eos)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [float(m0.sum()), float(m1.sum()), float(m2.sum())]
    e_m = float(((means.cpu().double() - means_ref.detach()).abs() / means_ref.detach().abs()).max())
    e_d = maxrel(d_loss, x.grad)
    report("lm_loss_summaries R 6400", means_rel=e_m, d_loss=e_d)
    assert e_m < FWD and e_d < GRAD


# ---- 6. the remaining small kernels -------------------------------------------------------------------------------------------------

def test_spatial_max_fwd_bwd(H, dev):
    """cvcl_spatial_max_fwd / _bwd at HW = 256: a tied maximum over the locations goes to the first one, a maximum at p = 255 is
    representable in the uint8 arg; logits against float64 at 2e-5; d_mm is non-zero exactly at the selected entries and equals
    d_logits exp(nlt) / len there (1e-4 against float64); d_neg_log_temp = sum d_logits logits.  HW = 257 is refused."""
    Bi, HW, Bt, L = 3, 256, 5, 7
    ncol = Bt * L
    g = torch.Generator().manual_seed(9)
    mm = torch.randn(Bi, HW, ncol, generator=g)
    mm[:, 255, 0::5] = 7.0                                 # the maximum at the last location
    mm[:, 17, 1::5] = 6.0                                  # a tie of two locations: 17 wins
    mm[:, 200, 1::5] = 6.0
    mm[:, 0, 2::5] = 6.5                                   # a tie with location 0 (the kernel's starting value)
    mm[:, 255, 2::5] = 6.5
    ln = torch.tensor([7, 1, 3, 7, 5])
    nlt = torch.tensor([math.log(1 / 0.07)])
    d_logits = torch.randn(Bi, Bt, generator=g)
    arg_ref = torch.from_numpy(np.argmax(mm.numpy(), axis=1))                          # numpy: the first maximum
    assert bool((arg_ref[:, 0::5] == 255).all()) and bool((arg_ref[:, 1::5] == 17).all()) and bool((arg_ref[:, 2::5] == 0).all())
    m64, n64 = mm.double(), nlt.double()
    logits_ref = m64.max(1).values.reshape(Bi, Bt, L).sum(2) / ln.double() * n64.exp()
    mmd, lnd, nltd, d_logitsd = mm.to(dev), ln.to(dev), nlt.to(dev), d_logits.to(dev)
    logits, arg = nans(dev, Bi, Bt), torch.full((Bi, ncol), 99, dtype=torch.uint8, device=dev)
    run(H, "cvcl_spatial_max_fwd", H.ptr(mmd), H.ptr(lnd), H.ptr(nltd), H.ptr(logits), H.ptr(arg), Bi, HW, Bt, L)
    d_mm, d_nlt = nans(dev, Bi, HW, ncol), nans(dev, 1)
    run(H, "cvcl_spatial_max_bwd", H.ptr(d_logitsd), H.ptr(arg), H.ptr(lnd), H.ptr(nltd), H.ptr(logits), H.ptr(d_mm), H.ptr(d_nlt),
        Bi, HW, Bt, L)
    torch.cuda.synchronize()
    assert torch.equal(arg.cpu().long(), arg_ref)
    onehot = torch.zeros(Bi, HW, ncol, dtype=torch.bool).scatter_(1, arg_ref[:, None, :], True)
    # autograd's max sends the gradient of a tie to one of the tied entries of its own choosing: the reference gradient is written out
    d_mm_ref = onehot * (d_logits.double() * n64.detach().exp() / ln.double()).repeat_interleave(L, 1)[:, None, :]
    d_nlt_ref = (d_logits.double() * logits_ref.detach()).sum()
    assert torch.equal(d_mm.cpu() != 0, onehot)
    e = dict(logits=maxrel(logits, logits_ref), d_mm=maxrel(d_mm, d_mm_ref),
             d_nlt=abs(float(d_nlt) - float(d_nlt_ref)) / abs(float(d_nlt_ref)))
    report("spatial_max HW 256", **e)
    assert e["logits"] < FWD and e["d_mm"] < GRAD and e["d_nlt"] < GRAD
    logits2, arg2 = nans(dev, Bi, Bt), torch.full((Bi, ncol), 99, dtype=torch.uint8, device=dev)
    big = torch.zeros(Bi, 257, ncol, device=dev)
    rc = H.lib().cvcl_spatial_max_fwd(H.ptr(big), H.ptr(lnd), H.ptr(nltd), H.ptr(logits2), H.ptr(arg2), Bi, 257, Bt, L, H.stream_ptr())
    torch.cuda.synchronize()
    assert rc == EINVAL and bool(torch.isnan(logits2).all()) and bool((arg2 == 99).all())


@pytest.mark.parametrize("B,L,E,crange", [(3, 5, 8, 7), (3, 5, 8, 5), (4, 1, 6, 1), (2, 9, 5, 2)])
def test_cbow_vs_float64(H, dev, B, L, E, crange):
    """cvcl_cbow with a window wider than the sequence (crange >= L: every other position, over 2 crange), L = 1 (no neighbour: zeros)
    and an ordinary window."""
    x = torch.randn(B, L, E, generator=torch.Generator().manual_seed(L + crange))
    ref = torch.zeros(B, L, E, dtype=torch.float64)
    for j in range(L):
        for k in range(max(j - crange, 0), min(j + crange, L - 1) + 1):
            if k != j:
                ref[:, j] += x[:, k].double()
    ref /= 2 * crange
    y, xd = nans(dev, B, L, E), x.to(dev)
    run(H, "cvcl_cbow", H.ptr(xd), H.ptr(y), B, L, E, crange)
    torch.cuda.synchronize()
    if L == 1:
        assert bool((y == 0).all())
    else:
        e = maxrel(y, ref)
        report(f"cbow B {B} L {L} E {E} crange {crange}", y=e)
        assert e < FWD


def test_seq_reverse_is_exact_and_its_own_inverse(H, dev):
    B, L, E = 5, 6, 5
    ln = torch.tensor([1, 6, 3, 6, 2])
    x = torch.randn(B, L, E, generator=torch.Generator().manual_seed(4))
    ref = torch.zeros_like(x)
    for b in range(B):
        n = int(ln[b])
        ref[b, :n] = x[b, :n].flip(0)
    lnd, xd = ln.to(dev), x.to(dev)
    y, back = nans(dev, B, L, E), nans(dev, B, L, E)
    run(H, "cvcl_seq_reverse", H.ptr(xd), H.ptr(lnd), H.ptr(y), B, L, E)
    run(H, "cvcl_seq_reverse", H.ptr(y), H.ptr(lnd), H.ptr(back), B, L, E)
    torch.cuda.synchronize()
    valid = (torch.arange(L)[None, :] < ln[:, None])[:, :, None]
    assert torch.equal(y.cpu(), ref)
    assert torch.equal(back.cpu(), x * valid)


def test_gather_and_sequence_mean_past_the_grid_cap(H, dev):
    """cvcl_embed_gather_pos, cvcl_seq_sum_div and cvcl_seq_sum_div_bwd at B L E = 170 x 25 x 512 elements, more than the 8192 x 256 threads
    of their capped grids.  The gather (+ pos) is exact; ids -1, V and 5 + 2^32 give NaN rows; the mean over all L positions / len
    and its backward go against float64."""
    B, L, E, V = 170, 25, 512, 64
    assert B * L * E > CAP
    g = torch.Generator().manual_seed(8)
    table, pos = torch.randn(V, E, generator=g), torch.randn(L, E, generator=g)
    tok = torch.randint(0, V, (B, L), generator=g)
    ln = torch.randint(1, L + 1, (B,), generator=g)
    bad = {(0, 3): -1, (B - 1, L - 1): V, (100, 7): 5 + 2 ** 32}
    for (b, l), t in bad.items():
        tok[b, l] = t
    isbad = (tok < 0) | (tok >= V)
    assert int(isbad.sum()) == 3
    ref = table[tok.clamp(0, V - 1)] + pos[None]
    tokd, lnd, tabled, posd = tok.to(dev), ln.to(dev), table.to(dev), pos.to(dev)
    x = nans(dev, B, L, E)
    run(H, "cvcl_embed_gather_pos", H.ptr(tabled), H.ptr(tokd), H.ptr(posd), H.ptr(x), B, L, E, V)
    x0 = torch.zeros(B, L, E, device=dev)
    run(H, "cvcl_embed_gather_pos", H.ptr(tabled), H.ptr(tokd), None, H.ptr(x0), B, L, E, V)
    torch.cuda.synchronize()
    x, x0 = x.cpu(), x0.cpu()
    assert bool(torch.isnan(x[isbad]).all()) and bool(torch.isnan(x0[isbad]).all())
    assert torch.equal(x[~isbad], ref[~isbad]) and torch.equal(x0[~isbad], table[tok.clamp(0, V - 1)][~isbad])
    xin = ref.contiguous()                                # finite everywhere
    ret, d_x = nans(dev, B, E), nans(dev, B, L, E)
    d_ret = torch.randn(B, E, generator=g)
    xind, d_retd = xin.to(dev), d_ret.to(dev)
    run(H, "cvcl_seq_sum_div", H.ptr(xind), H.ptr(lnd), H.ptr(ret), B, L, E)
    run(H, "cvcl_seq_sum_div_bwd", H.ptr(d_retd), H.ptr(lnd), H.ptr(d_x), B, L, E)
    torch.cuda.synchronize()
    e = dict(ret=maxrel(ret, xin.double().sum(1) / ln[:, None].double()),
             d_x=maxrel(d_x, (d_ret.double() / ln[:, None].double())[:, None, :].expand(B, L, E)))
    report("seq_sum_div B 170 L 25 E 512", **e)
    assert e["ret"] < FWD and e["d_x"] < GRAD
