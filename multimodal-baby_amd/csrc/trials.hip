// Forced-choice trial scores (gfx950): every trial of an evaluation from two feature tables and an index table, in one launch.
// Replace, in eval.py of the reference:
//   :196-232  per trial `model(img, label, label_len)` -> `torch.softmax(logits, dim=-1)` -> `torch.argmax(logits)`, with the
//             4 images (or the 4 labels) of the trial encoded again for it
// Eval-mode encoders are per sample, so a frame or a word that takes part in many trials is encoded ONCE (multimodal/trials.py) and a
// trial is n dot products between rows of the two tables (include/cvcl_hip.h "Trial scores" gives the definitions).
//
// cvcl_trial_scores    a wave64 takes one trial (4 trials per 256-thread workgroup).  Lane l holds elements l, l + 64, ... of the
//                      query row in registers -- QK of them, a 64 QK-element slice of the row at a time -- and walks the trial's n
//                      candidate rows against them: one 256-byte load per wave and element column, no alignment needed beyond
//                      float, the rows read in place through their leading dimensions.  Per candidate a lane's products are added
//                      in ascending column order and the 64 partial sums go through one xor butterfly: the order depends on D
//                      alone, never on T, on the trial's place in the grid or on its neighbours.  After the butterfly every lane
//                      holds all n logits; each evaluates the soft-max (maximum subtracted, terms added in candidate order) and the
//                      arg-max (the lowest position of the maximum), and lane j stores column j.  No LDS, no atomics, no workspace.
//                      The indices are device data: a trial with an index outside its table reads no row at all and is written as
//                      NaN / -1.
#include "cvcl_common.h"

namespace {

constexpr int TW = 4;                            // trials (waves) per workgroup
constexpr int QK = 8;                            // query elements a lane holds at a time: slices of 64 QK = 512 columns
constexpr int NMAX = CVCL_TRIAL_MAX_CHOICES;
static_assert(NMAX <= 64, "lane j stores column j");

__global__ __launch_bounds__(TW * 64) void trial_scores_kernel(const float* __restrict__ query, long ldq, int Nq,
                                                               const float* __restrict__ cand, long ldc, int Nc, int D,
                                                               const int32_t* __restrict__ q_idx, const int32_t* __restrict__ c_idx,
                                                               int T, int n, const float* __restrict__ log_scale,
                                                               float* __restrict__ logits, float* __restrict__ probs,
                                                               int32_t* __restrict__ pred) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * TW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (wave-uniform)
    if (t >= T) return;
    // the trial's rows; one index outside its table and no row of the trial is read
    const int qi = q_idx[t];
    bool ok = qi >= 0 && qi < Nq;
    int ci[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        ci[j] = j < n ? c_idx[t * n + j] : 0;
        ok = ok && ci[j] >= 0 && ci[j] < Nc;
    }
    if (!ok) {
        if (lane < n) {
            const float bad = __builtin_nanf("");
            if (logits) logits[t * n + lane] = bad;
            probs[t * n + lane] = bad;
        }
        if (lane == 0) pred[t] = -1;
        return;
    }
    const float* qrow = query + (long)qi * ldq;
    float acc[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) acc[j] = 0.f;
    for (long d0 = 0; d0 < D; d0 += 64 * QK) {
        float q[QK];
#pragma unroll
        for (int k = 0; k < QK; ++k) {
            const long d = d0 + 64 * k + lane;
            q[k] = d < D ? qrow[d] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < n) {                                         // (wave-uniform)
                const float* crow = cand + (long)ci[j] * ldc;
                float c[QK];
#pragma unroll
                for (int k = 0; k < QK; ++k) {                   // the slice's loads are in flight together
                    const long d = d0 + 64 * k + lane;
                    c[k] = d < D ? crow[d] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < QK; ++k) acc[j] = fmaf(q[k], c[k], acc[j]);      // (a column past D adds 0 * 0)
            }
        }
    }
    const float scale = log_scale ? expf(*log_scale) : 1.f;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        if (j < n) {
            acc[j] = scale * wave_sum(acc[j]);                   // (xor butterfly: every lane ends with the same bits)
            m = fmaxf(m, acc[j]);
        }
    }
    float e[NMAX], s = 0.f;
    int best = -1;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        e[j] = 0.f;
        if (j < n) {
            e[j] = expf(acc[j] - m);
            s += e[j];
            if (best < 0 && acc[j] == m) best = j;               // the lowest position of the maximum (-1 only if a logit is NaN)
        }
    }
    float mine_l = 0.f, mine_e = 0.f;                            // column `lane` without a dynamically indexed register array
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        mine_l = lane == j ? acc[j] : mine_l;
        mine_e = lane == j ? e[j] : mine_e;
    }
    if (lane < n) {
        if (logits) logits[t * n + lane] = mine_l;
        probs[t * n + lane] = mine_e / s;
    }
    if (lane == 0) pred[t] = best;
}

}  // namespace

extern "C" int cvcl_trial_scores(const float* query, long ldq, int Nq, const float* cand, long ldc, int Nc, int D, const int32_t* q_idx,
                                 const int32_t* c_idx, int T, int n, const float* log_scale, float* logits, float* probs, int32_t* pred,
                                 void* stream) {
    CVCL_CHECK_ARG(query, "cvcl_trial_scores: null pointer (query)");
    CVCL_CHECK_ARG(cand, "cvcl_trial_scores: null pointer (cand)");
    CVCL_CHECK_ARG(q_idx, "cvcl_trial_scores: null pointer (q_idx)");
    CVCL_CHECK_ARG(c_idx, "cvcl_trial_scores: null pointer (c_idx)");
    CVCL_CHECK_ARG(probs, "cvcl_trial_scores: null pointer (probs)");
    CVCL_CHECK_ARG(pred, "cvcl_trial_scores: null pointer (pred)");
    CVCL_CHECK_ARG(n >= 1 && n <= CVCL_TRIAL_MAX_CHOICES, "cvcl_trial_scores: n %d outside 1..%d", n, CVCL_TRIAL_MAX_CHOICES);
    CVCL_CHECK_ARG(D >= 1, "cvcl_trial_scores: D %d < 1", D);
    CVCL_CHECK_ARG(ldq >= D, "cvcl_trial_scores: ldq %ld < D %d", ldq, D);
    CVCL_CHECK_ARG(ldc >= D, "cvcl_trial_scores: ldc %ld < D %d", ldc, D);
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_trial_scores: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nc >= 1, "cvcl_trial_scores: Nc %d < 1", Nc);
    CVCL_CHECK_ARG(T >= 0, "cvcl_trial_scores: T %d < 0", T);
    if (T == 0) return CVCL_OK;
    CvclProfScope prof(stream, CVCL_K_HEAD);
    trial_scores_kernel<<<cvcl_div_up(T, TW), TW * 64, 0, (hipStream_t)stream>>>(query, ldq, Nq, cand, ldc, Nc, D, q_idx, c_idx, T, n, log_scale,
                                                                                  logits, probs, pred);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
