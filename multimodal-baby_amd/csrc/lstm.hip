// LSTM step kernels (gate order i,f,g,o; nn.LSTM): the forward cell of the text encoder (reference multimodal/multimodal.py:513-552),
// of the captioning LM and of the beam-search decode, and the BPTT step of all three backward sweeps (training, the captioning
// state, the per-word Grad-CAM seeds).  The cell's arithmetic is written once, forward and backward; the kernels differ only in
// where their rows come from and go to.  All fp32, deterministic (no atomics).
#include "cvcl_common.h"

#include <math.h>

namespace {

// ---- the cell, per element ----------------------------------------------------------------------
// pre-activations (a_i, a_f, a_g, a_o) and c_{t-1} -> gate activations, c_t, h_t
__device__ __forceinline__ void lstm_cell_fwd(float a_i, float a_f, float a_g, float a_o, float c_prev, float& ig, float& fg, float& gg,
                                              float& og, float& cn, float& ho) {
    ig = 1.f / (1.f + expf(-a_i));
    fg = 1.f / (1.f + expf(-a_f));
    gg = tanhf(a_g);
    og = 1.f / (1.f + expf(-a_o));
    cn = fg * c_prev + ig * gg;
    ho = og * tanhf(cn);
}

// gate activations, c_t, c_{t-1}, dho (gradient wrt h_t), dcv (gradient wrt c_t from the steps after) -> the pre-activation gate
// gradients and the gradient wrt c_{t-1}
__device__ __forceinline__ void lstm_cell_bwd(float ig, float fg, float gg, float og, float c_t, float c_prev, float dho, float dcv,
                                              float& d_i, float& d_f, float& d_g, float& d_o, float& dc_prev) {
    const float tc = tanhf(c_t);
    const float dct = dcv + dho * og * (1.f - tc * tc);
    d_i = dct * gg * ig * (1.f - ig);
    d_f = dct * c_prev * fg * (1.f - fg);
    d_g = dct * ig * (1.f - gg * gg);
    d_o = dho * tc * og * (1.f - og);
    dc_prev = dct * fg;
}

// V consecutive floats as one access (V = 4: 16 bytes)
template <int V> using fvec = float __attribute__((ext_vector_type(V)));
template <int V> __device__ __forceinline__ fvec<V> ldv(const float* p) { return *reinterpret_cast<const fvec<V>*>(p); }
template <int V> __device__ __forceinline__ void stv(float* p, fvec<V> v) { *reinterpret_cast<fvec<V>*>(p) = v; }

// ---- forward ------------------------------------------------------------------------------------
// LSTM cell for step t: gates [B,4H] already = x_t W_ih^T + b_ih + b_hh + h W_hh^T.  Sequences shorter than t+1 keep their state
// (packed-sequence semantics) and emit zeros (pad_packed_sequence).  Training saves for BPTT in [B, L, .] layout (row b*L + t,
// matching the rows of the input-projection GEMM): gate activations, c_t, h_{t-1}; the three save pointers are NULL for inference.
__global__ __launch_bounds__(256) void lstm_cell_kernel(const float* __restrict__ gates, const int64_t* __restrict__ len, int t,
                                                        float* __restrict__ h, float* __restrict__ c, float* __restrict__ out,
                                                        float* __restrict__ gates_act, float* __restrict__ c_save,
                                                        float* __restrict__ h_prev_save, int B, int L, int Hd) {
    const long total = (long)B * Hd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % Hd);
        const long b = i / Hd;
        const long row = b * L + t;
        if (h_prev_save) h_prev_save[row * Hd + j] = h[i];
        float ho = 0.f;
        if (len[b] > t) {
            const float* gp = gates + b * 4 * Hd;
            float ig, fg, gg, og, cn;
            lstm_cell_fwd(gp[j], gp[Hd + j], gp[2 * Hd + j], gp[3 * Hd + j], c[i], ig, fg, gg, og, cn, ho);
            if (gates_act) {
                float* ga = gates_act + row * 4 * Hd;
                ga[j] = ig; ga[Hd + j] = fg; ga[2 * Hd + j] = gg; ga[3 * Hd + j] = og;
            }
            c[i] = cn;
            h[i] = ho;
        }
        if (c_save) c_save[row * Hd + j] = c[i];
        if (out) out[row * Hd + j] = ho;
    }
}

// LSTM cell of one decode step on N beam rows: gates [N, 4H] = h W_hh^T, G [V, 4H] = table W_ih^T + b_ih + b_hh; the row of each
// beam's input token is added before the cell.  h, c updated in place.
__global__ __launch_bounds__(256) void lstm_cell_tok_kernel(const float* __restrict__ gates, const float* __restrict__ G,
                                                            const int64_t* __restrict__ tok, int V, float* __restrict__ h,
                                                            float* __restrict__ c, int N, int Hd) {
    const long total = (long)N * Hd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % Hd);
        const long n = i / Hd;
        const int64_t t = tok[n];
        if (t < 0 || t >= V) continue;                // not a token of the vocabulary: the row keeps its state
        const float* gp = gates + n * 4 * Hd;
        const float* gr = G + t * 4 * Hd;
        float ig, fg, gg, og, cn, ho;
        lstm_cell_fwd(gp[j] + gr[j], gp[Hd + j] + gr[Hd + j], gp[2 * Hd + j] + gr[2 * Hd + j], gp[3 * Hd + j] + gr[3 * Hd + j], c[i], ig,
                      fg, gg, og, cn, ho);
        c[i] = cn;
        h[i] = ho;
    }
}

// ---- backward -----------------------------------------------------------------------------------
// BPTT step s on `rows` gradient rows, V hidden units per lane.  Row r belongs to sequence r % B and reads that sequence's saved row
// b L + s; c_{s-1} is the saved row before it, or c0 (zeros if NULL) at s = 0.  In: dh (gradient wrt h_s), dc (gradient wrt c_s,
// updated in place to the gradient wrt c_{s-1}).  Out: the pre-activation gate gradients in row r * dg_stride + dg_first of d_gates,
// dh_carry = dh for rows whose step was not taken (their h_s = h_{s-1}), 0 otherwise.
//   training (rows = B): row b L + s of the [B, L, 4H] buffer, dg_stride = L, dg_first = s
//   per-word Grad-CAM (rows = a multiple of B, seed-major [L][B][H]: block p holds the chains that started at position p, so the
//   chains alive at step s are a contiguous tail): row r of a [rows, 4H] buffer, dg_stride = 1, dg_first = 0.  d_out != NULL: the
//   first B rows are the chains that start at this step -- their dh is d_out[b L + s] (0 where the sequence has ended) and their dc
//   is 0, neither buffer is read for them.
template <int V>
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ gates_act, const float* __restrict__ c_save,
                                                            const float* __restrict__ c0, const int64_t* __restrict__ len, int s,
                                                            const float* __restrict__ d_out, const float* __restrict__ dh,
                                                            float* __restrict__ dc, float* __restrict__ d_gates, long dg_stride,
                                                            long dg_first, float* __restrict__ dh_carry, int B, int L, int Hd,
                                                            long rows) {
    const int Hq = Hd / V;
    const long total = rows * Hq;
    static_assert(V == 1 || V == 4, "one float or one 16-byte access per lane");
    const fvec<V> zero = (fvec<V>)0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % Hq) * V;
        const long r = i / Hq;
        const int b = (int)(r % B);
        const long srow = (long)b * L + s;
        const long off = r * Hd + j;
        const bool joins = d_out != nullptr && r < B;
        const bool live = len[b] > s;
        float* dg = d_gates + (r * dg_stride + dg_first) * 4 * Hd + j;
        if (!live) {                                 // the step was not taken: h_s = h_{s-1}, c_s = c_{s-1}
            stv<V>(dg, zero); stv<V>(dg + Hd, zero); stv<V>(dg + 2 * Hd, zero); stv<V>(dg + 3 * Hd, zero);
            stv<V>(dh_carry + off, joins ? zero : ldv<V>(dh + off));
            if (joins) stv<V>(dc + off, zero);
            continue;
        }
        const fvec<V> dho = joins ? ldv<V>(d_out + srow * Hd + j) : ldv<V>(dh + off);
        const fvec<V> dcv = joins ? zero : ldv<V>(dc + off);
        const float* ga = gates_act + srow * 4 * Hd + j;
        const fvec<V> ig = ldv<V>(ga), fg = ldv<V>(ga + Hd), gg = ldv<V>(ga + 2 * Hd), og = ldv<V>(ga + 3 * Hd);
        const fvec<V> c_t = ldv<V>(c_save + srow * Hd + j);
        const fvec<V> c_prev = s > 0 ? ldv<V>(c_save + (srow - 1) * Hd + j) : (c0 ? ldv<V>(c0 + (long)b * Hd + j) : zero);
        fvec<V> d_i, d_f, d_g, d_o, dcn;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float di, df, dg_, do_, dcp;
            lstm_cell_bwd(ig[e], fg[e], gg[e], og[e], c_t[e], c_prev[e], dho[e], dcv[e], di, df, dg_, do_, dcp);
            d_i[e] = di; d_f[e] = df; d_g[e] = dg_; d_o[e] = do_; dcn[e] = dcp;
        }
        stv<V>(dg, d_i); stv<V>(dg + Hd, d_f); stv<V>(dg + 2 * Hd, d_g); stv<V>(dg + 3 * Hd, d_o);
        stv<V>(dc + off, dcn);
        stv<V>(dh_carry + off, zero);
    }
}

// dh[b][:] += d_out[b][t][:] for the sequences still running at step t (out[b][t] = h_t there, 0 beyond the length): lets
// the per-step outputs of the LSTM (the language-model branch, multimodal.py:859) take part in the BPTT
__global__ __launch_bounds__(256) void lstm_add_dout_kernel(float* __restrict__ dh, const float* __restrict__ d_out,
                                                            const int64_t* __restrict__ len, int t, int B, int L, int Hd) {
    const long total = (long)B * Hd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / Hd;
        const int j = (int)(i % Hd);
        if (len[b] > t) dh[i] += d_out[(b * L + t) * Hd + j];
    }
}

// y[b][t] = x[b][len[b]-1-t] for t < len[b], 0 beyond: the backward direction of a packed bidirectional LSTM runs over each
// sequence from its last valid token; the same permutation un-reverses its outputs (and is its own adjoint)
__global__ __launch_bounds__(256) void seq_reverse_kernel(const float* __restrict__ x, const int64_t* __restrict__ len,
                                                          float* __restrict__ y, int B, int L, int E) {
    const long total = (long)B * L * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const long r = i / E;
        const int t = (int)(r % L);
        const long b = r / L;
        const int n = (int)len[b];
        y[i] = t < n ? x[(b * L + (n - 1 - t)) * E + e] : 0.f;
    }
}

}  // namespace

// ================================================================================================
extern "C" int cvcl_lstm_cell(const float* gates, const int64_t* len, int t, float* h, float* c, float* out, int B, int L,
                              int Hd, void* stream) {
    CVCL_CHECK_ARG(gates && len && h && c && B > 0 && L > 0 && Hd > 0 && t >= 0 && t < L, "cvcl_lstm_cell: bad args");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_kernel, dim3(cvcl_grid((long)B * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, gates, len, t, h,
                       c, out, (float*)nullptr, (float*)nullptr, (float*)nullptr, B, L, Hd);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_lstm_cell_train(const float* gates, const int64_t* len, int t, float* h, float* c, float* out,
                                    float* gates_act, float* c_save, float* h_prev_save, int B, int L, int Hd, void* stream) {
    CVCL_CHECK_ARG(gates && len && h && c && gates_act && c_save && h_prev_save && B > 0 && L > 0 && Hd > 0 && t >= 0 && t < L,
                   "cvcl_lstm_cell_train: bad args");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_kernel, dim3(cvcl_grid((long)B * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, gates, len, t, h,
                       c, out, gates_act, c_save, h_prev_save, B, L, Hd);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_lstm_cell_tok(const float* gates, const float* G, const int64_t* tok, int V, float* h, float* c, int N, int Hd,
                                  void* stream) {
    CVCL_CHECK_ARG(N >= 1 && Hd >= 1 && V >= 1, "cvcl_lstm_cell_tok: bad sizes");
    CVCL_CHECK_ARG(gates && G && tok && h && c, "cvcl_lstm_cell_tok: null pointer");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_tok_kernel, dim3(cvcl_grid((long)N * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, gates, G, tok,
                       V, h, c, N, Hd);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_lstm_cell_bwd(const float* gates_act, const float* c_save, const int64_t* len, int t, const float* dh,
                                  float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd, void* stream) {
    CVCL_CHECK_ARG(gates_act && c_save && len && dh && dc && d_gates && dh_carry && B > 0 && L > 0 && Hd > 0 && t >= 0 && t < L,
                   "cvcl_lstm_cell_bwd: bad args");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<1>, dim3(cvcl_grid((long)B * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, gates_act,
                       c_save, (const float*)nullptr, len, t, (const float*)nullptr, dh, dc, d_gates, (long)L,
                       (long)t, dh_carry, B, L, Hd, (long)B);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// BPTT step t = 0 of an LSTM that started from (h0, c0) (the captioning state): cvcl_lstm_cell_bwd with c_{-1} = c0 instead of
// zeros.  dc is updated in place to the gradient wrt c0; dh_carry as there.
extern "C" int cvcl_lstm_cell_bwd_first(const float* gates_act, const float* c_save, const float* c0, const int64_t* len,
                                        const float* dh, float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd,
                                        void* stream) {
    CVCL_CHECK_ARG(B >= 1 && L >= 1 && Hd >= 1, "cvcl_lstm_cell_bwd_first: bad sizes");
    CVCL_CHECK_ARG(gates_act && c_save && c0 && len && dh && dc && d_gates && dh_carry, "cvcl_lstm_cell_bwd_first: null pointer");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<1>, dim3(cvcl_grid((long)B * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, gates_act,
                       c_save, c0, len, 0, (const float*)nullptr, dh, dc, d_gates, (long)L, 0L, dh_carry, B, L, Hd,
                       (long)B);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// The multi-seed BPTT sweep of the per-word Grad-CAM (include/cvcl_hip.h "Per-word Grad-CAM"): every (caption, word) pair is one
// seed row whose gradient chain runs over the SAME saved gate activations of its caption, so one launch + one recurrent GEMM serve
// all the chains alive at step s.  Four hidden units per lane.
extern "C" int cvcl_lstm_cell_bwd_seeds(const float* gates_act, const float* c_save, const float* c0, const int64_t* len, int s,
                                        const float* d_out, float* dh, float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd,
                                        long rows, void* stream) {
    CVCL_CHECK_ARG(gates_act && c_save && len && dh && dc && d_gates && dh_carry, "cvcl_lstm_cell_bwd_seeds: null pointer");
    CVCL_CHECK_ARG(B >= 1 && L >= 1, "cvcl_lstm_cell_bwd_seeds: bad sizes (B %d, L %d)", B, L);
    CVCL_CHECK_ARG(Hd >= 4 && Hd % 4 == 0, "cvcl_lstm_cell_bwd_seeds: Hd %d is not a positive multiple of 4", Hd);
    CVCL_CHECK_ARG(s >= 0 && s < L, "cvcl_lstm_cell_bwd_seeds: step %d outside [0, %d)", s, L);
    CVCL_CHECK_ARG(rows >= 1 && rows % B == 0, "cvcl_lstm_cell_bwd_seeds: rows %ld is not a positive multiple of B %d", rows, B);
    CVCL_CHECK_ARG(rows / B <= L - s, "cvcl_lstm_cell_bwd_seeds: %ld seed blocks at step %d, at most %d can be alive", rows / B, s, L - s);
    CVCL_CHECK_ARG(!c0 || s == 0, "cvcl_lstm_cell_bwd_seeds: c0 belongs to step 0 (step %d)", s);
    CVCL_CHECK_ARG(cvcl_aligned16(gates_act) && cvcl_aligned16(c_save) && cvcl_aligned16(c0) && cvcl_aligned16(d_out) &&
                   cvcl_aligned16(dh) && cvcl_aligned16(dc) && cvcl_aligned16(d_gates) && cvcl_aligned16(dh_carry),
                   "cvcl_lstm_cell_bwd_seeds: a buffer is not 16-byte aligned");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<4>, dim3(cvcl_grid(rows * (Hd / 4), 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       gates_act, c_save, c0, len, s, d_out, dh, dc, d_gates, 1L, 0L, dh_carry, B, L, Hd, rows);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_lstm_add_dout(float* dh, const float* d_out, const int64_t* len, int t, int B, int L, int Hd, void* stream) {
    CVCL_CHECK_ARG(dh && d_out && len && B > 0 && L > 0 && Hd > 0 && t >= 0 && t < L, "cvcl_lstm_add_dout: bad args");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(lstm_add_dout_kernel, dim3(cvcl_grid((long)B * Hd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, dh, d_out, len,
                       t, B, L, Hd);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_seq_reverse(const float* x, const int64_t* len, float* y, int B, int L, int E, void* stream) {
    CVCL_CHECK_ARG(x && len && y && x != y && B > 0 && L > 0 && E > 0, "cvcl_seq_reverse: bad args");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    hipLaunchKernelGGL(seq_reverse_kernel, dim3(cvcl_grid((long)B * L * E, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, len, y, B,
                       L, E);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
