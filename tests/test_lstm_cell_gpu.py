"""GPU: the LSTM step entries of csrc/lstm.hip against each other, through the C ABI.  The forward cell and the BPTT step are each
written once there and every entry calls them, so the entries agree bit for bit where their definitions overlap:

- cvcl_lstm_cell and cvcl_lstm_cell_train leave the same h, c and out, and the training one saves c_t and h_{t-1};
- cvcl_lstm_cell_tok on a token of the vocabulary is cvcl_lstm_cell on gates + G[tok], and leaves any other row alone;
- cvcl_lstm_cell_bwd_first with c0 = 0 is cvcl_lstm_cell_bwd at t = 0, at a hidden size that is no multiple of 4 (the multiples of
  4 are covered against cvcl_lstm_cell_bwd_seeds in test_caption_gradcam_gpu.py).

Every comparison is torch.equal: no arithmetic differs between the two sides, so there is no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, L = 3, 4
LENS = [4, 2, 0]                                      # live throughout, ends mid-sequence, never runs


def _lens():
    return torch.as_tensor(LENS, dtype=torch.int64).to(DEV)


# Hd 6: no multiple of 4, 18 work items; Hd 260: 780 items, three full 256-thread blocks and a tail
@pytest.mark.parametrize("Hd", [6, 260])
def test_cell_equals_cell_train(Hd):
    from multimodal import _hip as H
    lib, st = H.lib(), H.stream_ptr()
    g = torch.Generator().manual_seed(Hd)
    h0, c0 = torch.randn(B, Hd, generator=g).to(DEV), torch.randn(B, Hd, generator=g).to(DEV)
    gates = torch.randn(L, B, 4 * Hd, generator=g).to(DEV)
    ln = _lens()
    h_i, c_i, out_i = h0.clone(), c0.clone(), torch.full((B, L, Hd), float("nan"), device=DEV)
    h_t, c_t, out_t = h0.clone(), c0.clone(), torch.full((B, L, Hd), float("nan"), device=DEV)
    gact = torch.full((B * L, 4 * Hd), float("nan"), device=DEV)
    c_save = torch.full((B * L, Hd), float("nan"), device=DEV)
    h_prev = torch.full((B * L, Hd), float("nan"), device=DEV)
    for t in range(L):
        h_before, c_before = h_t.clone(), c_t.clone()
        H.check(lib.cvcl_lstm_cell(H.ptr(gates[t]), H.ptr(ln), t, H.ptr(h_i), H.ptr(c_i), H.ptr(out_i), B, L, Hd, st), "cvcl_lstm_cell")
        H.check(lib.cvcl_lstm_cell_train(H.ptr(gates[t]), H.ptr(ln), t, H.ptr(h_t), H.ptr(c_t), H.ptr(out_t), H.ptr(gact), H.ptr(c_save),
                                         H.ptr(h_prev), B, L, Hd, st), "cvcl_lstm_cell_train")
        torch.cuda.synchronize()
        assert torch.equal(h_i, h_t) and torch.equal(c_i, c_t)
        assert torch.equal(out_i[:, t], out_t[:, t]) and not torch.isnan(out_t[:, t]).any()
        assert torch.equal(c_save.view(B, L, Hd)[:, t], c_t)
        assert torch.equal(h_prev.view(B, L, Hd)[:, t], h_before)
        live = ln > t
        assert torch.equal(h_t[~live], h_before[~live]) and torch.equal(c_t[~live], c_before[~live])   # packed-sequence semantics
        assert bool((out_t[:, t][~live] == 0).all()) and torch.equal(out_t[:, t][live], h_t[live])
        assert not torch.isnan(gact.view(B, L, -1)[:, t][live]).any()
    assert not torch.equal(h_t[0], h0[0]) and torch.equal(h_t[2], h0[2]) and torch.equal(c_t[2], c0[2])


def test_cell_tok_equals_cell_on_gathered_rows():
    from multimodal import _hip as H
    lib, st = H.lib(), H.stream_ptr()
    N, Hd, V = 5, 6, 7
    g = torch.Generator().manual_seed(1)
    tok = torch.tensor([0, 6, 3, -1, 7], dtype=torch.int64).to(DEV)                            # the last two are no tokens of the vocabulary
    gates = torch.randn(N, 4 * Hd, generator=g).to(DEV)
    G = torch.randn(V, 4 * Hd, generator=g).to(DEV)
    h0, c0 = torch.randn(N, Hd, generator=g).to(DEV), torch.randn(N, Hd, generator=g).to(DEV)
    h, c = h0.clone(), c0.clone()
    H.check(lib.cvcl_lstm_cell_tok(H.ptr(gates), H.ptr(G), H.ptr(tok), V, H.ptr(h), H.ptr(c), N, Hd, st), "cvcl_lstm_cell_tok")
    summed = (gates[:3] + G[tok[:3]]).contiguous()                                             # one fp32 add per element, as in the kernel
    h_w, c_w = h0[:3].clone(), c0[:3].clone()
    ones = torch.ones(3, dtype=torch.int64, device=DEV)
    H.check(lib.cvcl_lstm_cell(H.ptr(summed), H.ptr(ones), 0, H.ptr(h_w), H.ptr(c_w), None, 3, 1, Hd, st), "cvcl_lstm_cell")
    torch.cuda.synchronize()
    assert torch.equal(h[:3], h_w) and torch.equal(c[:3], c_w)
    assert not torch.equal(h[:3], h0[:3])
    assert torch.equal(h[3:], h0[3:]) and torch.equal(c[3:], c0[3:])


def _bwd_inputs(Hd, seed):
    g = torch.Generator().manual_seed(seed)
    gact = torch.rand(B * L, 4 * Hd, generator=g)
    gact[:, 2 * Hd:3 * Hd] = gact[:, 2 * Hd:3 * Hd] * 2 - 1                                     # the cell gate is a tanh
    csave = torch.randn(B * L, Hd, generator=g)
    dh, dc = torch.randn(B, Hd, generator=g), torch.randn(B, Hd, generator=g)
    return gact.to(DEV), csave.to(DEV), dh.to(DEV), dc.to(DEV)


def _cell_bwd(H, gact, csave, ln, t, dh, dc, Hd, c0=None):
    lib, st = H.lib(), H.stream_ptr()
    dc = dc.clone()
    dG = torch.full((B * L, 4 * Hd), float("nan"), device=DEV)
    carry = torch.full((B, Hd), float("nan"), device=DEV)
    if c0 is None:
        H.check(lib.cvcl_lstm_cell_bwd(H.ptr(gact), H.ptr(csave), H.ptr(ln), t, H.ptr(dh), H.ptr(dc), H.ptr(dG), H.ptr(carry), B, L, Hd,
                                       st), "cvcl_lstm_cell_bwd")
    else:
        H.check(lib.cvcl_lstm_cell_bwd_first(H.ptr(gact), H.ptr(csave), H.ptr(c0), H.ptr(ln), H.ptr(dh), H.ptr(dc), H.ptr(dG),
                                             H.ptr(carry), B, L, Hd, st), "cvcl_lstm_cell_bwd_first")
    torch.cuda.synchronize()
    return dG.view(B, L, 4 * Hd), carry, dc


def test_cell_bwd_first_with_zero_c0_equals_cell_bwd_scalar_width():
    from multimodal import _hip as H
    Hd = 6
    gact, csave, dh, dc = _bwd_inputs(Hd, seed=2)
    ln = _lens()
    dG_w, carry_w, dc_w = _cell_bwd(H, gact, csave, ln, 0, dh, dc, Hd)
    dG, carry, dc_g = _cell_bwd(H, gact, csave, ln, 0, dh, dc, Hd, c0=torch.zeros(B, Hd, device=DEV))
    assert not torch.isnan(dG[:, 0]).any() and torch.isnan(dG[:, 1:]).all()                    # row b L + t and no other
    assert torch.equal(dG[:, 0], dG_w[:, 0]) and torch.equal(carry, carry_w) and torch.equal(dc_g, dc_w)
    assert bool((dG[:2, 0] != 0).any()) and bool((dG[2, 0] == 0).all())


def test_cell_bwd_masks_ended_rows():
    from multimodal import _hip as H
    Hd = 6
    gact, csave, dh, dc = _bwd_inputs(Hd, seed=3)
    ln = _lens()
    dG, carry, dc_g = _cell_bwd(H, gact, csave, ln, 2, dh, dc, Hd)
    ended = ln <= 2
    assert ended.tolist() == [False, True, True]
    assert not torch.isnan(dG[:, 2]).any() and bool((dG[:, 2][ended] == 0).all()) and bool((dG[:, 2][~ended] != 0).any())
    assert torch.equal(carry[ended], dh[ended]) and bool((carry[~ended] == 0).all())
    assert torch.equal(dc_g[ended], dc[ended])
