"""GPU: H.gemm on row-strided views (H.rows) hands cvcl_gemm the block the LSTM paths used to fill by hand, refuses what is not such a
view before anything is enqueued, and ops.lstm_recurrence is the one loop behind ops.lstm_text and text_train.LstmCore.

Shapes (B, L, H): (5, 7, 32) and (130, 3, 36) -- L > 1 (the leading dimension differs from the width), t > 0 (a non-zero offset);
the second crosses a 128-row and a 128-column tile edge with a K that is no multiple of the 64-deep step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 32), (130, 3, 36)]
TOL = 2e-5                                                  # test_gemm_gpu.py's fp32 bound, in its metric
SENTINEL = -777.0


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    return _hip


def _rel(y, ref):
    err = (y.double().cpu() - ref).abs()
    return float((err / (ref.abs() + ref.abs().max() * 5e-2)).max())


def _operands(B, L, Hd, dev):
    g = torch.Generator().manual_seed(B * 1000 + L * 100 + Hd)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"h": r(B, Hd).to(dev), "w_hh": (r(4 * Hd, Hd) / Hd ** 0.5).to(dev), "gx": r(B * L, 4 * Hd).to(dev),
            "dG": r(B * L, 4 * Hd).to(dev), "carry": r(B, Hd).to(dev)}


def _raw_gemm(H, fill):
    a = H.GemmArgs()
    fill(a)
    H.check(H.lib().cvcl_gemm(H.F32, a, H.stream_ptr()), "cvcl_gemm")


@pytest.mark.parametrize("B,L,Hd", SHAPES)
def test_forward_step_is_the_hand_written_block(H, dev, B, L, Hd):
    """gates = h W_hh^T + gx[:, t] through the view == the block ops.lstm_text filled by hand, bit for bit, and float64."""
    d = _operands(B, L, Hd, dev)
    h, w_hh, gx = d["h"], d["w_hh"], d["gx"]
    for t in range(L):
        gates = torch.full((B, 4 * Hd), SENTINEL, device=dev)
        H.gemm(h, w_hh, residual=gx.view(B, L, 4 * Hd)[:, t], out=gates)
        by_hand = torch.full((B, 4 * Hd), SENTINEL, device=dev)

        def fill(a):
            a.A, a.W, a.C = H.ptr(h), H.ptr(w_hh), H.ptr(by_hand)
            a.M, a.N, a.K, a.lda, a.ldw, a.ldc = B, 4 * Hd, Hd, Hd, Hd, 4 * Hd
            a.R, a.ldr = gx.data_ptr() + t * 4 * Hd * 4, L * 4 * Hd
        _raw_gemm(H, fill)
        assert torch.equal(gates, by_hand), t
        ref = h.double().cpu() @ w_hh.double().cpu().t() + gx.view(B, L, 4 * Hd)[:, t].double().cpu()
        rel = _rel(gates, ref)
        print(f"forward B={B} L={L} H={Hd} t={t}: rel {rel:.3e}")
        assert rel < TOL, t


@pytest.mark.parametrize("B,L,Hd", SHAPES)
def test_backward_step_is_the_hand_written_block(H, dev, B, L, Hd):
    """dh = dG[:, t] W_hh + carry into rows r0 .. r0 + B of a larger buffer == LstmCore.backward's hand-filled block; the rows
    outside the slice keep their sentinel."""
    d = _operands(B, L, Hd, dev)
    w_hh, dG, carry = d["w_hh"], d["dG"], d["carry"]
    r0 = 3
    for t in range(L):
        buf = torch.full((B + 7, Hd), SENTINEL, device=dev)
        H.gemm(dG.view(B, L, 4 * Hd)[:, t], w_hh, w_trans=True, residual=carry, out=buf[r0:r0 + B])
        by_hand = torch.full((B, Hd), SENTINEL, device=dev)

        def fill(a):
            a.A, a.W, a.C = dG.data_ptr() + t * 4 * Hd * 4, H.ptr(w_hh), H.ptr(by_hand)
            a.M, a.N, a.K, a.lda, a.ldw, a.ldc = B, Hd, 4 * Hd, L * 4 * Hd, Hd, Hd
            a.w_trans = 1
            a.R, a.ldr = H.ptr(carry), Hd
        _raw_gemm(H, fill)
        assert torch.equal(buf[r0:r0 + B], by_hand), t
        assert bool((buf[:r0] == SENTINEL).all()) and bool((buf[r0 + B:] == SENTINEL).all()), t
        ref = dG.view(B, L, 4 * Hd)[:, t].double().cpu() @ w_hh.double().cpu() + carry.double().cpu()
        rel = _rel(by_hand, ref)
        print(f"backward B={B} L={L} H={Hd} t={t}: rel {rel:.3e}")
        assert rel < TOL, t


def test_refusals_leave_out_untouched(H, dev):
    B, L, Hd = 5, 7, 32
    d = _operands(B, L, Hd, dev)
    h, w_hh, gx = d["h"], d["w_hh"], d["gx"]
    N = 4 * Hd
    gx_t = gx.view(B, L, N)[:, 1]
    out = torch.full((B, N), SENTINEL, device=dev)
    wide = torch.randn(B, 2 * Hd, device=dev)
    flat = torch.randn(B * N, device=dev)
    cases = {
        "column-strided A": dict(A=wide[:, ::2]),
        "column-strided residual": dict(residual=torch.randn(B, 2 * N, device=dev)[:, ::2]),
        "row stride below the width": dict(residual=torch.as_strided(flat, (B, N), (N // 2, 1))),
        "out of the wrong dtype": dict(out=torch.full((B, N), SENTINEL, dtype=torch.bfloat16, device=dev)),
        "out too short": dict(out=torch.full((B - 1, N), SENTINEL, device=dev)),
        "out of the wrong width": dict(out=torch.full((B, N + 4), SENTINEL, device=dev)),
        "residual of the wrong width": dict(residual=torch.randn(B, L, N + 4, device=dev)[:, 1]),
        "residual too short": dict(residual=gx_t[:B - 1]),
    }
    for name, kw in cases.items():
        args = dict(A=h, residual=gx_t, out=out)
        args.update(kw)
        before = args["out"].clone()
        with pytest.raises(H.CvclError):
            H.gemm(args["A"], w_hh, residual=args["residual"], out=args["out"])
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and torch.equal(args["out"], before), name
    for name, kw in {"A": dict(A=h.cpu()), "W": dict(W=w_hh.cpu()), "residual": dict(residual=gx_t.cpu()),
                     "out": dict(out=torch.full((B, N), SENTINEL))}.items():
        args = dict(A=h, W=w_hh, residual=gx_t, out=out)
        args.update(kw)
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            H.gemm(args["A"], args["W"], residual=args["residual"], out=args["out"])
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((args["out"] == SENTINEL).all()), name
    with pytest.raises(H.CvclError, match="no CPU fallback"):
        H.rows(gx_t.cpu())
    with pytest.raises(H.CvclError):
        H.rows(gx_t, torch.bfloat16)
    assert H.rows(gx_t) == (gx.data_ptr() + N * 4, L * N) and H.rows(gx[2:3]) == (gx.data_ptr() + 2 * N * 4, N)


def test_recurrence_is_one_loop(H, dev):
    """save=False / save=True (the two cell kernels) leave identical h, c and out, and ops.lstm_text is bit for bit
    text_train.LstmCore's forward on the same weights: both are ops.lstm_recurrence."""
    from multimodal import ops
    from multimodal.text_train import LstmCore
    B, L, Hd = 5, 7, 32
    E, V = Hd, 50
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(E, Hd, batch_first=True).to(dev)
    table = torch.randn(V, E, device=dev)
    tok = torch.randint(1, V, (B, L), device=dev)
    length = torch.tensor([7, 1, 4, 6, 2], device=dev)
    h0, c0 = torch.randn(B, Hd, device=dev), torch.randn(B, Hd, device=dev)
    with torch.no_grad():
        x = ops._embed_gather(table, tok)
        gx = H.gemm(x, lstm.weight_ih_l0.contiguous(), bias=(lstm.bias_ih_l0 + lstm.bias_hh_l0).contiguous())
        w_hh = lstm.weight_hh_l0.detach().contiguous()
        s0 = ops.lstm_initial_state(h0, c0, B, Hd, dev)
        s1 = ops.lstm_initial_state(h0, c0, B, Hd, dev)
        out0 = ops.lstm_recurrence(gx, w_hh, length, s0, B, L)
        out1, gact, csave, hprev = ops.lstm_recurrence(gx, w_hh, length, s1, B, L, save=True)
        assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
        assert torch.equal(out0, out1)                      # (zeros beyond each sequence's length, from both kernels)
        assert gact.shape == (B * L, 4 * Hd) and csave.shape == hprev.shape == (B * L, Hd)
        for state in ((None, None), (h0, c0)):
            h_e, out_e = ops.lstm_text(table, lstm, tok, length, *state)
            h_t, out_t = LstmCore.apply(x, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, length, B, L, *state)
            assert torch.equal(h_e, h_t) and torch.equal(out_e, out_t[:, :int(length.max())])
    with pytest.raises(ValueError, match="both h0 and c0 or neither"):
        ops.lstm_initial_state(h0, None, B, Hd, dev)
