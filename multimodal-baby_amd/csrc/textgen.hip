// Beam-search text generation (include/cvcl_hip.h "Beam-search decoding"): one launch per decode step does one inner_loop of the
// reference's beam search (multimodal/beam_search.py:418-611) for every batch item, with the stop test (:613-667) evaluated on the
// device, so a decode runs without a host sync until its end.  The cell of a decode step (cvcl_lstm_cell_tok: the gathered input-
// projection row of the previous token added, then the LSTM cell on all B K beam rows) is in csrc/lstm.hip.  All arithmetic is fp32.
#include "cvcl_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CVCL_WAVE;
constexpr float kInf = 1e7f;                          // beam_search.py INF: the penalty added to unfinished / finished scores

// One workgroup per batch item b.  M: per-lane candidate list length (>= 2K).
template <int M>
__global__ __launch_bounds__(kThreads) void beam_step_kernel(
    const float* __restrict__ logits, int B, int K, int V, int T, int step, float lp, float max_lp, int eos_id,
    const float* __restrict__ alive_lp_in, float* __restrict__ alive_lp_out, const float* __restrict__ fin_in,
    float* __restrict__ fin_out, int64_t* __restrict__ alive_seq, int64_t* __restrict__ fin_seq, int32_t* __restrict__ fin_flags,
    const float* __restrict__ h_in, const float* __restrict__ c_in, float* __restrict__ h_out, float* __restrict__ c_out, int Hd,
    int64_t* __restrict__ next_tok, int32_t* __restrict__ steps) {
    __shared__ float s_lse[16], s_alp[16];
    __shared__ float s_red_s[2][kWaves];
    __shared__ int s_red_i[2][kWaves];
    __shared__ float s_cs[32];                        // the 2K candidates in order: score, flat index
    __shared__ int s_ci[32];
    __shared__ int s_apar[16], s_atok[16];            // new alive beam k: parent beam, appended token
    __shared__ int s_fsrc[16], s_fpar[16], s_ftok[16]; // new finished beam k: old finished slot (or -1), else parent / token
    __shared__ int64_t s_aseq[16 * (CVCL_BEAM_MAX_T + 1)], s_fseq[16 * (CVCL_BEAM_MAX_T + 1)];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long bk = (long)b * K;

    // ---- stop test (_is_finished, stop_early): one decision over the whole batch, from the state before this step.  Nothing in
    // this launch writes the *_in buffers, so every workgroup reaches the same answer; a stopped decode stays stopped (its state
    // is carried over unchanged), so later launches repeat the decision and only copy.
    int met = 1;
    for (int i = tid; i < B; i += kThreads) {
        float best = fin_in[(long)i * K];
        for (int k = 1; k < K; ++k) best = fmaxf(best, fin_in[(long)i * K + k]);
        met &= best > alive_lp_in[(long)i * K] / max_lp;
    }
    const bool stop = __syncthreads_and(met) || step >= T;
    if (stop) {
        if (tid < K) {
            alive_lp_out[bk + tid] = alive_lp_in[bk + tid];
            fin_out[bk + tid] = fin_in[bk + tid];
        }
        if (b == 0 && tid == 0) atomicMin(steps, step);
        return;
    }

    // ---- stage the sequences of this item (columns 0..step) before anything is overwritten
    const int cols = step + 1, ld = T + 1;
    for (int e = tid; e < K * cols; e += kThreads) {
        const int k = e / cols, j = e - k * cols;
        s_aseq[k * cols + j] = alive_seq[(bk + k) * ld + j];
        s_fseq[k * cols + j] = fin_seq[(bk + k) * ld + j];
    }

    // ---- pass 1: per-beam log-sum-exp, one wave per beam
    const float* lg = logits + bk * V;
    for (int k = w; k < K; k += kWaves) {
        const float* row = lg + (long)k * V;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
        m = wave_max(m);
        const float mm = isinf(m) ? 0.f : m;
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf(row[v] - mm);
        s = wave_sum(s);
        if (lane == 0) {
            s_lse[k] = logf(s) + mm;
            s_alp[k] = alive_lp_in[bk + k];
        }
    }
    __syncthreads();

    // ---- pass 2: per-lane top-M lists of the K V length-penalised scores, then 2K rounds of a workgroup arg-max over the heads
    float ls[M];
    int li[M];
#pragma unroll
    for (int j = 0; j < M; ++j) { ls[j] = -INFINITY; li[j] = 0x7fffffff; }
    const int KV = K * V;
    for (int f = tid; f < KV; f += kThreads) {
        const int k = f / V;
        const float s = ((lg[f] - s_lse[k]) + s_alp[k]) / lp;
        if (cvcl_better(s, f, ls[M - 1], li[M - 1])) {
            ls[M - 1] = s;
            li[M - 1] = f;
#pragma unroll
            for (int j = M - 1; j > 0; --j) {
                if (cvcl_better(ls[j], li[j], ls[j - 1], li[j - 1])) {
                    const float ts = ls[j]; ls[j] = ls[j - 1]; ls[j - 1] = ts;
                    const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
                }
            }
        }
    }
    const int K2 = 2 * K;
    for (int r = 0; r < K2; ++r) {
        float bs = ls[0];
        int bi = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (cvcl_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { s_red_s[r & 1][w] = bs; s_red_i[r & 1][w] = bi; }
        __syncthreads();
        bs = s_red_s[r & 1][0];
        bi = s_red_i[r & 1][0];
#pragma unroll
        for (int q = 1; q < kWaves; ++q)
            if (cvcl_better(s_red_s[r & 1][q], s_red_i[r & 1][q], bs, bi)) { bs = s_red_s[r & 1][q]; bi = s_red_i[r & 1][q]; }
        if (tid == 0) { s_cs[r] = bs; s_ci[r] = bi; }
        if (li[0] == bi) {                            // flat indices are unique: exactly one lane owned the winner
#pragma unroll
            for (int j = 0; j < M - 1; ++j) { ls[j] = ls[j + 1]; li[j] = li[j + 1]; }
            ls[M - 1] = -INFINITY;
            li[M - 1] = 0x7fffffff;
        }
    }
    __syncthreads();

    // ---- grow_alive / grow_finished on the 2K candidates (tiny: one lane)
    if (tid == 0) {
        bool taken[48];
        for (int j = 0; j < 3 * K; ++j) taken[j] = false;
        // grow_alive: top K of score + flag * -INF
        for (int k = 0; k < K; ++k) {
            int bj = -1;
            float bv = 0.f;
            for (int r = 0; r < K2; ++r) {
                if (taken[r]) continue;
                const bool fin = s_ci[r] % V == eos_id;
                const float v = s_cs[r] + (fin ? -kInf : -0.f);
                if (bj < 0 || cvcl_better(v, r, bv, bj)) { bj = r; bv = v; }
            }
            taken[bj] = true;
            s_apar[k] = s_ci[bj] / V;
            s_atok[k] = s_ci[bj] % V;
            alive_lp_out[bk + k] = s_cs[bj] * lp;     // topk_log_probs = topk_scores * length_penalty
        }
        // grow_finished: top K of [finished K ; candidates 2K + (1 - flag) * -INF]
        for (int j = 0; j < 3 * K; ++j) taken[j] = false;
        int oldflag[16];
        for (int k = 0; k < K; ++k) oldflag[k] = fin_flags[bk + k];
        for (int k = 0; k < K; ++k) {
            int bj = -1;
            float bv = 0.f;
            for (int j = 0; j < 3 * K; ++j) {
                if (taken[j]) continue;
                float v;
                if (j < K) {
                    v = fin_in[bk + j];
                } else {
                    const bool fin = s_ci[j - K] % V == eos_id;
                    v = s_cs[j - K] + (fin ? -0.f : -kInf);
                }
                if (bj < 0 || cvcl_better(v, j, bv, bj)) { bj = j; bv = v; }
            }
            taken[bj] = true;
            fin_out[bk + k] = bv;
            if (bj < K) {
                s_fsrc[k] = bj;
                s_fpar[k] = 0;
                s_ftok[k] = 0;
                fin_flags[bk + k] = oldflag[bj];
            } else {
                s_fsrc[k] = -1;
                s_fpar[k] = s_ci[bj - K] / V;
                s_ftok[k] = s_ci[bj - K] % V;
                fin_flags[bk + k] = s_ftok[k] == eos_id;
            }
        }
    }
    __syncthreads();

    // ---- writes: sequences gathered by parent with the token appended, state rows gathered by parent, next input tokens
    const int cols2 = cols + 1;
    for (int e = tid; e < K * cols2; e += kThreads) {
        const int k = e / cols2, j = e - k * cols2;
        alive_seq[(bk + k) * ld + j] = j < cols ? s_aseq[s_apar[k] * cols + j] : (int64_t)s_atok[k];
        int64_t v;
        if (s_fsrc[k] >= 0) v = j < cols ? s_fseq[s_fsrc[k] * cols + j] : 0;
        else v = j < cols ? s_aseq[s_fpar[k] * cols + j] : (int64_t)s_ftok[k];
        fin_seq[(bk + k) * ld + j] = v;
    }
    if (tid < K) next_tok[bk + tid] = s_atok[tid];
    for (long e = tid; e < (long)K * Hd; e += kThreads) {
        const int k = (int)(e / Hd);
        const long j = e - (long)k * Hd;
        const long src = (bk + s_apar[k]) * Hd + j, dst = (bk + k) * Hd + j;
        h_out[dst] = h_in[src];
        c_out[dst] = c_in[src];
    }
}

// The reference's per-item fallback (beam_search.py:683-703): an item with no finished flag returns its alive sequences and
// log-probs, any other its finished sequences and scores.
__global__ __launch_bounds__(kThreads) void beam_finalize_kernel(int K, int T, const int64_t* __restrict__ alive_seq,
                                                                 const float* __restrict__ alive_lp, const int64_t* __restrict__ fin_seq,
                                                                 const float* __restrict__ fin_scores, const int32_t* __restrict__ fin_flags,
                                                                 int64_t* __restrict__ out_seq, float* __restrict__ out_scores) {
    const long bk = (long)blockIdx.x * K;
    bool any = false;
    for (int k = 0; k < K; ++k) any |= fin_flags[bk + k] != 0;
    const int64_t* seq = any ? fin_seq : alive_seq;
    const float* sc = any ? fin_scores : alive_lp;
    const long n = (long)K * (T + 1);
    for (long e = threadIdx.x; e < n; e += kThreads) out_seq[bk * (T + 1) + e] = seq[bk * (T + 1) + e];
    if ((int)threadIdx.x < K) out_scores[bk + threadIdx.x] = sc[bk + threadIdx.x];
}


}  // namespace

extern "C" int cvcl_beam_step(const float* logits, int B, int K, int V, int T, int step, double alpha, int eos_id,
                              const float* alive_lp_in, float* alive_lp_out, const float* fin_scores_in, float* fin_scores_out,
                              int64_t* alive_seq, int64_t* fin_seq, int32_t* fin_flags, const float* h_in, const float* c_in,
                              float* h_out, float* c_out, int Hd, int64_t* next_tok, int32_t* steps, void* stream) {
    CVCL_CHECK_ARG(K >= 1 && K <= CVCL_BEAM_MAX_K, "cvcl_beam_step: beam width %d outside [1, %d]", K, CVCL_BEAM_MAX_K);
    CVCL_CHECK_ARG(2 * K <= V, "cvcl_beam_step: 2K = %d exceeds the vocabulary size %d", 2 * K, V);
    CVCL_CHECK_ARG(T >= 1 && T <= CVCL_BEAM_MAX_T, "cvcl_beam_step: decode length %d outside [1, %d]", T, CVCL_BEAM_MAX_T);
    CVCL_CHECK_ARG(B >= 1 && Hd >= 1 && step >= 0 && step < T && (long)K * V < 0x7fffffffL, "cvcl_beam_step: bad sizes");
    CVCL_CHECK_ARG(logits && alive_lp_in && alive_lp_out && fin_scores_in && fin_scores_out && alive_seq && fin_seq && fin_flags &&
                   h_in && c_in && h_out && c_out && next_tok && steps, "cvcl_beam_step: null pointer");
    CVCL_CHECK_ARG(alive_lp_in != alive_lp_out && fin_scores_in != fin_scores_out && h_in != h_out && c_in != c_out,
                   "cvcl_beam_step: the *_in and *_out buffers must differ (ping-pong pairs)");
    // length penalties as the reference forms them: Python floats, rounded to fp32 where they meet the fp32 scores
    const float lp = (float)pow((5.0 + (double)(step + 1)) / 6.0, alpha);
    const float max_lp = (float)pow((5.0 + (double)T) / 6.0, alpha);
    CvclProfScope prof(stream, CVCL_K_HEAD);
#define CVCL_BEAM_LAUNCH(M)                                                                                                      \
    hipLaunchKernelGGL(beam_step_kernel<M>, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, logits, B, K, V, T, step, lp, max_lp, \
                       eos_id, alive_lp_in, alive_lp_out, fin_scores_in, fin_scores_out, alive_seq, fin_seq, fin_flags, h_in, c_in, \
                       h_out, c_out, Hd, next_tok, steps)
    if (K <= 4) CVCL_BEAM_LAUNCH(8);
    else if (K <= 8) CVCL_BEAM_LAUNCH(16);
    else CVCL_BEAM_LAUNCH(32);
#undef CVCL_BEAM_LAUNCH
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_beam_finalize(int B, int K, int T, const int64_t* alive_seq, const float* alive_lp, const int64_t* fin_seq,
                                  const float* fin_scores, const int32_t* fin_flags, int64_t* out_seq, float* out_scores,
                                  void* stream) {
    CVCL_CHECK_ARG(B >= 1 && K >= 1 && K <= CVCL_BEAM_MAX_K && T >= 1 && T <= CVCL_BEAM_MAX_T, "cvcl_beam_finalize: bad sizes");
    CVCL_CHECK_ARG(alive_seq && alive_lp && fin_seq && fin_scores && fin_flags && out_seq && out_scores,
                   "cvcl_beam_finalize: null pointer");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, K, T, alive_seq, alive_lp, fin_seq,
                       fin_scores, fin_flags, out_seq, out_scores);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
