// Nearest-neighbour searches between two frame sets (gfx950): arg-max cosine similarity of feature rows and arg-min L1 distance of
// 8-bit frames.  Replace the torch compositions of analysis_cvcl/duplicates.py in the reference:
//   :561-612  F.cosine_similarity on broadcast operands per category, then np.argmax / np.max per evaluation frame
//   :795-838  F.cosine_similarity(eval[:, None, :], train[None, :, :]) + torch.max / torch.argmax (the 1-NN classifier)
//   :988-1002 torch.sum(torch.abs(eval_img - train_images), dim=(1, 2, 3)) + torch.min / torch.argmin, batch by batch
// Neither search writes a queries x base matrix: every workgroup keeps a running (best value, index) per query in registers over
// the base tiles it owns, the workgroups of one query tile leave their partial results in the caller's workspace, and a second
// small kernel merges them in a fixed order (no atomics: results are reproducible; ties go to the lower index everywhere).
//
// cvcl_nn_cosine   128 queries x 128 base rows per 256-thread workgroup (4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles), K in
//                  steps of 32 through LDS (144-byte row pitch, as csrc/gemm.hip), products on v_mfma_f32_32x32x2_f32 (exact fp32).
//                  The accumulators are emptied into a second set every 128 k: the running sum of a chain then stays 16x smaller
//                  than the result, and the rounding of the sum stays at the fp32 class of a pairwise sum (an arg-max among
//                  near-duplicates needs it: their cosines sit within 1e-3 of 1).  Row norms come from a pass of their own, in
//                  double; cos = float(double(dot) / (max(|q|, eps) max(|b|, eps))), one rounding.
// cvcl_knn_cosine  the same device function (cosine_tile_walk) with another tile epilogue: a sorted list of k per (split, query) in the
//                  workspace instead of one running best, so a pair's cosine has cvcl_nn_cosine's bits by construction;
//                  cvcl_knn_vote sums exp(cos / T) per class over such lists (section "k nearest neighbours" below).
// cvcl_rank_cosine the walk's third epilogue: per query the number of negatives (base rows of another key) that beat a given
//                  threshold (the query's best positive, which cvcl_nn_cosine found with the keys as groups), an integer counter per
//                  lane and query, so the position of the best positive among all base rows costs no list and no matrix.
// cvcl_nn_l1_u8    each WAVE owns TQ x TB (8 x 8) frame pairs: its lanes stride over the pixel dwords of one channel, every lane
//                  holds TQ + TB loaded 16-byte pieces and TQ TB accumulators, so each loaded dword feeds TB (or TQ) v_sad_u8.
//                  At the end of a channel a transposing wave reduction (63 exchanges for 64 sums) leaves the total of pair l in
//                  lane l; the distance is formed in double there, left to right over the channels.
#include "cvcl_common.h"

namespace {

constexpr size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ================================================================================================================================
// cosine
// ================================================================================================================================
constexpr int CT = 128;              // tile edge (queries and base rows)
constexpr int CBK = 32;              // k per LDS step
constexpr int CROWB = 144;           // LDS row pitch in bytes (128 B of k + 16 B pad)
constexpr int CFLUSH = 4;            // k steps per accumulator chain (128 k)
constexpr int kCosineTargetWgs = 512;        // 2 workgroups per CU on 256 CUs

struct CosDev {
    const float* q; const float* b;
    int ldq, ldb, Nq, Nb, D;
    const double* invq; const double* invb;
    const int32_t* qg; const int32_t* bg;
    float* pval; int32_t* pidx;       // [splits][Nq]
    int nbt;                          // base tiles
    int vec;                          // rows are 16-byte aligned and D % 4 == 0
};

// 1 / max(|x_r|, eps) in double, one wave per row (fixed xor tree: deterministic)
__global__ __launch_bounds__(256) void nn_inv_norm_kernel(const float* __restrict__ x, int ld, int N, int D, float eps,
                                                          double* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* r = x + (long)row * ld;
    double s = 0.0;
    for (int k = lane; k < D; k += 64) { const double v = (double)r[k]; s += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = 1.0 / fmax(sqrt(s), (double)eps);
}

__global__ __launch_bounds__(256) void nn_cosine_merge_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx, int splits,
                                                              int Nq, long idx_offset, int accumulate, float* __restrict__ best_cos,
                                                              int64_t* __restrict__ best_idx) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nq) return;
    float bv = -INFINITY;
    long bi = -1;
    if (accumulate) { bv = best_cos[m]; bi = best_idx[m]; }
    for (int s = 0; s < splits; ++s) {
        const float v = pval[(long)s * Nq + m];
        const int i = pidx[(long)s * Nq + m];
        if (i < 0) continue;
        const long gi = idx_offset + i;
        if (bi < 0 || v > bv || (v == bv && gi < bi)) { bv = v; bi = gi; }
    }
    best_cos[m] = bv;
    best_idx[m] = bi;
}

int cosine_splits(int Nq, int Nb) {
    const int qtiles = cvcl_div_up(Nq, CT), nbt = cvcl_div_up(Nb, CT);
    int s = kCosineTargetWgs / qtiles;
    if (s < 1) s = 1;
    return s < nbt ? s : nbt;
}

// ================================================================================================================================
// the tile walk of both cosine searches, the lists of the k nearest, and the vote over them
// ================================================================================================================================
// nn_cosine_kernel and knn_cosine_kernel are one tile walk (cosine_tile_walk below: staging, MFMA products, chains, scaling), so a
// pair's cosine has the same bits in both, and k = 1 of cvcl_knn_cosine is cvcl_nn_cosine's result.  What differs is the epilogue
// of a tile.  Each (split, query) owns one sorted list of k (value, row) pairs in the workspace, empty slots (-inf, -1) at
// its end, and its k-th entry -- the threshold -- and its fill count in LDS.  The tile's cosines go to LDS in two halves of 64 base
// rows (the staging area is free then); wave w takes queries 32 w .. 32 w + 31 of the tile, reads the 64 candidates of one query,
// one per lane, and where the ballot of "the list is not full, or this beats the threshold" is not empty, merges them BY RANK: a
// live candidate's new position is the number of list entries and live candidates that beat it, an entry moves down by the number
// of candidates that beat it, and whatever lands below k is stored.  That is one read and one write of the list per (query, half tile) however many
// candidates enter: at most 64 wave-uniform steps of at most 5 ballots, which also bounds the worst case (rows arriving in ascending
// similarity).  A query's list is only ever touched by one wave, and at most once between two barriers of the LDS hand-over.
constexpr int KNN_PITCH = 68;                    // floats per LDS row of a half tile (64 + 4: 16-byte stores, rows on different banks)
constexpr int KNN_SLOTS = CVCL_KNN_MAX_K / 64;   // list entries a lane holds during a merge
static_assert(CT * KNN_PITCH * 4 <= 2 * CT * CROWB, "a half tile of cosines fits in the staging area");

struct KnnDev : CosDev {                         // pval / pidx: the lists, [splits][Nq][k]
    int k;
};

struct RankDev : CosDev {                        // qg / bg: the keys; pidx: the counts, [splits][Nq]; pval is not used
    const float* thr_cos; const int64_t* thr_idx;
    long idx_offset;
};

enum { WALK_ARGMAX = 0, WALK_TOPK = 1, WALK_RANK = 2 };      // what becomes of a finished tile

template <typename I>
__device__ __forceinline__ bool knn_better(float v, I i, float bv, I bi) {      // (bitwise: three compares, no branches)
    return (bool)((int)(v > bv) | ((int)(v == bv) & (int)(i < bi)));
}

// the value lane `src` (wave-uniform) holds
__device__ __forceinline__ int knn_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float knn_lane(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}
__device__ __forceinline__ long long knn_lane(long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave merges its live candidates (one per lane: `live`, value cv, row ci; `mask` is the ballot of `live`, not empty) into the
// sorted list lv / li [k], of which *cnt entries are held (the rest are empty and are not read).  Every held entry is read before any
// is written (the positions depend on all of them).  A step costs one ballot per 64 held entries and one for the candidates, so an
// empty list is filled at one ballot per candidate.  The pair that lands on position k - 1 is the new threshold.  Rows are distinct,
// so (value desc, row asc) is a total order and the positions are too.  The caller orders a later merge of the same list behind this
// one's stores (a barrier, or a fence for a list in LDS).
template <typename I>
__device__ __forceinline__ void knn_wave_merge(float* lv, I* li, int k, bool live, float cv, I ci, unsigned long long mask, int lane,
                                               float* thr_v, I* thr_i, int* cnt) {
    const int count = __builtin_amdgcn_readfirstlane(*cnt);
    const int nslots = (count + 63) >> 6, nlive = __popcll(mask);
    float ev[KNN_SLOTS];
    I ei[KNN_SLOTS];
    int er[KNN_SLOTS];
#pragma unroll
    for (int j = 0; j < KNN_SLOTS; ++j) {
        const int p = lane + 64 * j;
        er[j] = p;
        ev[j] = p < count ? lv[p] : -INFINITY;
        ei[j] = p < count ? li[p] : (I)-1;
    }
    int cr = 0;
    while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const float xv = knn_lane(cv, src);          // (v_readlane: src is wave-uniform)
        const I xi = knn_lane(ci, src);
        int ahead = 0;                               // entries and candidates that beat candidate `src`
#pragma unroll
        for (int j = 0; j < KNN_SLOTS; ++j) {
            if (j < nslots) {                        // (wave-uniform)
                // an empty slot holds -inf and never wins (a live candidate is above -inf); its position is not used
                const bool wins = knn_better<I>(ev[j], ei[j], xv, xi);
                ahead += __popcll(__builtin_amdgcn_ballot_w64(wins));
                er[j] += wins ? 0 : 1;
            }
        }
        // a candidate that is not live is -inf or below the threshold of a full list: it beats no live one
        ahead += __popcll(__builtin_amdgcn_ballot_w64(knn_better<I>(cv, ci, xv, xi)));
        cr = lane == src ? ahead : cr;
    }
#pragma unroll
    for (int j = 0; j < KNN_SLOTS; ++j) {
        if (ei[j] >= 0 && er[j] < k) {
            if (er[j] != lane + 64 * j) { lv[er[j]] = ev[j]; li[er[j]] = ei[j]; }
            if (er[j] == k - 1) { *thr_v = ev[j]; *thr_i = ei[j]; }
        }
    }
    if (live && cr < k) {
        lv[cr] = cv;
        li[cr] = ci;
        if (cr == k - 1) { *thr_v = cv; *thr_i = ci; }
    }
    if (lane == 0) *cnt = min(k, count + nlive);
}

// The tile walk of the cosine searches: this workgroup's query tile against the base tiles blockIdx.y, + gridDim.y, ...  MODE
// chooses what becomes of a finished tile: the running best per lane (WALK_ARGMAX, cvcl_nn_cosine; reduced over lane halves and waves
// and written per split at the end), the sorted lists of `topk` entries (WALK_TOPK, cvcl_knn_cosine; s_thr_v / s_thr_i / s_cnt [CT] in
// LDS are the lists' thresholds and fill counts, null otherwise), or the count per lane of the negatives that beat the query's
// threshold (WALK_RANK, cvcl_rank_cosine; reduced and written as the running best is).  Everything up to tot[][] is one piece of code
// for all three, which is why a pair's cosine has the same bits in each, whatever k, split or chunk -- and why comparing a cosine of
// the rank count with a threshold the arg-max search produced is meaningful.
template <bool VEC, int MODE, typename Dev>
__device__ __forceinline__ void cosine_tile_walk(const Dev& p, int topk, float* s_thr_v, int* s_thr_i, int* s_cnt) {
    constexpr bool TOPK = MODE == WALK_TOPK;
    __shared__ __attribute__((aligned(16))) char smem[2 * CT * CROWB];
    char* sQ = smem;
    char* sB = smem + CT * CROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, h = lane >> 5;
    const int kc = tid & 7, r0 = tid >> 3;           // staging role: 16-byte chunk kc of rows r0 + 32 j
    const int m0 = blockIdx.x * CT;
    const int ktiles = (p.D + CBK - 1) / CBK;
    const int my_tiles = (int)blockIdx.y < p.nbt ? (p.nbt - 1 - (int)blockIdx.y) / (int)gridDim.y + 1 : 0;
    const long steps = (long)my_tiles * ktiles;

    if constexpr (TOPK) {
        // wave w owns the lists of queries m0 + 32 w .. + 31: empty, no threshold
        if (lane < 32) { s_thr_v[wave * 32 + lane] = -INFINITY; s_thr_i[wave * 32 + lane] = -1; s_cnt[wave * 32 + lane] = 0; }
        for (int qq = 0; qq < 32; ++qq) {
            const int m = m0 + wave * 32 + qq;
            if (m >= p.Nq) break;
            const long o = ((long)blockIdx.y * p.Nq + m) * topk;
            for (int e = lane; e < topk; e += 64) { p.pval[o + e] = -INFINITY; p.pidx[o + e] = -1; }
        }
        __threadfence_block();
    }

    long q_off[4];
    bool q_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + r0 + 32 * j;
        q_ok[j] = m < p.Nq;
        q_off[j] = (long)m * p.ldq;
    }
    f32x4 tq[4], tb[4];
    auto issue = [&](long s) {                       // global -> registers for step s; rows / k beyond the operands read as 0
        const int bt = blockIdx.y + (int)(s / ktiles) * gridDim.y, kt = (int)(s % ktiles);
        const int k = kt * CBK + kc * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = bt * CT + r0 + 32 * j;
            const bool b_ok = n < p.Nb;
            const float* qr = p.q + q_off[j] + k;
            const float* br = p.b + (long)n * p.ldb + k;
            if (VEC) {
                tq[j] = (q_ok[j] && k < p.D) ? *reinterpret_cast<const f32x4*>(qr) : f32x4{0.f, 0.f, 0.f, 0.f};
                tb[j] = (b_ok && k < p.D) ? *reinterpret_cast<const f32x4*>(br) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tq[j][e] = (q_ok[j] && k + e < p.D) ? qr[e] : 0.f;
                    tb[j][e] = (b_ok && k + e < p.D) ? br[e] : 0.f;
                }
            }
        }
    };

    // this lane's queries: m0 + wm 64 + mt 32 + l31, mt = 0, 1
    float best_v[2] = {-INFINITY, -INFINITY};        // (arg-max only)
    int best_i[2] = {-1, -1};
    double invq[2];
    int qg[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + wm * 64 + mt * 32 + l31;
        invq[mt] = m < p.Nq ? p.invq[m] : 0.0;
        qg[mt] = (p.qg && m < p.Nq) ? p.qg[m] : 0;
    }
    // (rank count only) the threshold of each query: its cosine, and its row inside this call's base rows, clamped to 0 .. Nb (a
    // row of an earlier chunk is below every row of this one, a row of a later chunk above); the count of a query without a
    // threshold is not read
    float thr_v[2] = {0.f, 0.f};
    int thr_n[2] = {0, 0};
    int beat[2] = {0, 0};
    if constexpr (MODE == WALK_RANK) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = m0 + wm * 64 + mt * 32 + l31;
            if (m < p.Nq) {
                const long t = (long)p.thr_idx[m] - p.idx_offset;
                thr_v[mt] = p.thr_cos[m];
                thr_n[mt] = t < 0 ? 0 : (t > (long)p.Nb ? p.Nb : (int)t);
            }
        }
    }

    if (steps > 0) issue(0);
    long s = 0;
    for (int t = 0; t < my_tiles; ++t) {
        const int nbase = (blockIdx.y + t * gridDim.y) * CT;
        f32x16 acc[2][2], tot[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }
        for (int kt = 0; kt < ktiles; ++kt, ++s) {
            __syncthreads();                         // the previous step's fragments (top-k: or the previous tile's cosines) are read
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                *reinterpret_cast<f32x4*>(sQ + (r0 + 32 * j) * CROWB + kc * 16) = tq[j];
                *reinterpret_cast<f32x4*>(sB + (r0 + 32 * j) * CROWB + kc * 16) = tb[j];
            }
            __syncthreads();
            if (s + 1 < steps) issue(s + 1);         // the next step's loads fly under the MFMAs
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // lane half h owns k = 4 (2 g + h) .. + 3 of the step and feeds element e to the e-th 32x32x2 product: the
                // contraction index may be permuted freely as long as both operands agree
                f32x4 fb[2], fq[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    fb[x] = *reinterpret_cast<const f32x4*>(sB + (wn * 64 + x * 32 + l31) * CROWB + (g * 2 + h) * 16);
                    fq[x] = *reinterpret_cast<const f32x4*>(sQ + (wm * 64 + x * 32 + l31) * CROWB + (g * 2 + h) * 16);
                }
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[nt][e], fq[mt][e], acc[nt][mt], 0, 0, 0);
            }
            if ((kt % CFLUSH) == CFLUSH - 1 || kt == ktiles - 1) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) { tot[i][j][e] += acc[i][j][e]; acc[i][j][e] = 0.f; }
            }
        }
        if constexpr (MODE == WALK_RANK) {
            // epilogue (rows as below): a negative -- a row of another key -- counts where it would stand before the threshold in
            // a stable descending sort
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int n = nbase + wn * 64 + nt * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
                    const bool n_ok = n < p.Nb;
                    const double ib = n_ok ? p.invb[n] : 0.0;
                    const int g = n_ok ? p.bg[n] : 0;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const float c = (float)((double)tot[nt][mt][e] * invq[mt] * ib);
                        beat[mt] += (int)(n_ok && g != qg[mt] && cvcl_better(c, n, thr_v[mt], thr_n[mt]));
                    }
                }
        } else if constexpr (MODE == WALK_ARGMAX) {
            // epilogue: element e of tile (nt, mt) is base row nbase + wn 64 + nt 32 + 8 (e >> 2) + 4 h + (e & 3) against query mt
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int n = nbase + wn * 64 + nt * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
                    const bool n_ok = n < p.Nb;
                    const double ib = n_ok ? p.invb[n] : 0.0;
                    const int g = (p.bg && n_ok) ? p.bg[n] : 0;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const float c = (float)((double)tot[nt][mt][e] * invq[mt] * ib);
                        if (n_ok && g == qg[mt] && cvcl_better(c, n, best_v[mt], best_i[mt])) { best_v[mt] = c; best_i[mt] = n; }
                    }
                }
        } else {
            // epilogue, base rows nbase + wn 64 + nt 32 + .. of both wn at a time: sC[query of the tile][wn 32 + row of the 32];
            // element e of tile (nt, mt) is row 8 (e >> 2) + 4 h + (e & 3) against query mt.  A pair that is not eligible goes in as
            // -inf.
            float* sC = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                __syncthreads();                     // the last step's fragments (nt = 1: the first half's candidates) are read
#pragma unroll
                for (int eg = 0; eg < 4; ++eg) {
                    double ib[4];
                    int g[4];
                    bool n_ok[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int n = nbase + wn * 64 + nt * 32 + 8 * eg + 4 * h + e;
                        n_ok[e] = n < p.Nb;
                        ib[e] = n_ok[e] ? p.invb[n] : 0.0;
                        g[e] = (p.bg && n_ok[e]) ? p.bg[n] : 0;
                    }
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        f32x4 c4;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float c = (float)((double)tot[nt][mt][eg * 4 + e] * invq[mt] * ib[e]);
                            c4[e] = (n_ok[e] && g[e] == qg[mt]) ? c : -INFINITY;
                        }
                        *reinterpret_cast<f32x4*>(sC + (wm * 64 + mt * 32 + l31) * KNN_PITCH + wn * 32 + 8 * eg + 4 * h) = c4;
                    }
                }
                __syncthreads();
                for (int qq = 0; qq < 32; ++qq) {
                    const int ql = wave * 32 + qq, m = m0 + ql;
                    if (m >= p.Nq) break;
                    const float c = sC[ql * KNN_PITCH + lane];
                    const int n = nbase + (lane >> 5) * 64 + nt * 32 + (lane & 31);
                    const float tv = s_thr_v[ql];
                    const int ti = s_thr_i[ql];
                    const bool live = c > -INFINITY && (ti < 0 || cvcl_better(c, n, tv, ti));
                    const unsigned long long mask = __ballot(live);
                    if (!mask) continue;
                    const long o = ((long)blockIdx.y * p.Nq + m) * topk;
                    knn_wave_merge<int>(p.pval + o, p.pidx + o, topk, live, c, n, mask, lane, s_thr_v + ql, s_thr_i + ql, s_cnt + ql);
                }
            }
        }
    }
    if constexpr (MODE == WALK_RANK) {
        // lane halves, then the two waves of a query half (through LDS), then one count per query and split
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) beat[mt] += __shfl_xor(beat[mt], 32, 64);
        __syncthreads();
        int* rc = reinterpret_cast<int*>(smem);                  // [2][128]
        if (h == 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) rc[wn * CT + wm * 64 + mt * 32 + l31] = beat[mt];
        }
        __syncthreads();
        if (tid < CT && m0 + tid < p.Nq) p.pidx[(long)blockIdx.y * p.Nq + m0 + tid] = rc[tid] + rc[CT + tid];
    } else if constexpr (MODE == WALK_ARGMAX) {
        // lane halves, then the two waves of a query half (through LDS), then one partial per query and split
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float ov = __shfl_xor(best_v[mt], 32, 64);
            const int oi = __shfl_xor(best_i[mt], 32, 64);
            if (oi >= 0 && cvcl_better(ov, oi, best_v[mt], best_i[mt])) { best_v[mt] = ov; best_i[mt] = oi; }
        }
        __syncthreads();
        float* rv = reinterpret_cast<float*>(smem);              // [2][128]
        int* ri = reinterpret_cast<int*>(smem + 2 * CT * 4);
        if (h == 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                rv[wn * CT + wm * 64 + mt * 32 + l31] = best_v[mt];
                ri[wn * CT + wm * 64 + mt * 32 + l31] = best_i[mt];
            }
        }
        __syncthreads();
        if (tid < CT && m0 + tid < p.Nq) {
            float v = rv[tid];
            int i = ri[tid];
            const float v1 = rv[CT + tid];
            const int i1 = ri[CT + tid];
            if (i1 >= 0 && cvcl_better(v1, i1, v, i)) { v = v1; i = i1; }
            p.pval[(long)blockIdx.y * p.Nq + m0 + tid] = v;
            p.pidx[(long)blockIdx.y * p.Nq + m0 + tid] = i;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void nn_cosine_kernel(CosDev p) {
    cosine_tile_walk<VEC, WALK_ARGMAX>(p, 1, nullptr, nullptr, nullptr);
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void rank_cosine_kernel(RankDev p) {
    cosine_tile_walk<VEC, WALK_RANK>(p, 1, nullptr, nullptr, nullptr);
}

// the splits' counts of a query, added in split order to what rank holds (accumulate) or to 0; -1 without a threshold
__global__ __launch_bounds__(256) void rank_cosine_merge_kernel(const int32_t* __restrict__ pcnt, int splits, int Nq,
                                                                const int64_t* __restrict__ thr_idx, int accumulate,
                                                                int64_t* __restrict__ rank) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nq) return;
    if (thr_idx[m] < 0) { rank[m] = -1; return; }
    int64_t r = accumulate ? rank[m] : 0;
    for (int s = 0; s < splits; ++s) r += pcnt[(long)s * Nq + m];
    rank[m] = r;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void knn_cosine_kernel(KnnDev p) {
    __shared__ float s_thr_v[CT];                    // per query of the tile: its list's k-th entry (the threshold) and fill count
    __shared__ int s_thr_i[CT];
    __shared__ int s_cnt[CT];
    cosine_tile_walk<VEC, WALK_TOPK>(p, p.k, s_thr_v, s_thr_i, s_cnt);
}

// one wave per query: the result list is built in LDS from the previous outputs (accumulate) and the splits' lists, split by split.
// A split's list is sorted, so its first block of 64 without a live candidate ends it.
__global__ __launch_bounds__(256) void knn_cosine_merge_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx, int splits,
                                                               int Nq, int k, long idx_offset, int accumulate, float* top_cos,
                                                               int64_t* top_idx) {
    __shared__ float s_v[4][CVCL_KNN_MAX_K];
    __shared__ long long s_i[4][CVCL_KNN_MAX_K];
    __shared__ float s_thr_v[4];
    __shared__ long long s_thr_i[4];
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wave;
    if (m >= Nq) return;                             // (whole waves; no barrier below)
    float* rv = s_v[wave];
    long long* ri = s_i[wave];
    const long o = (long)m * k;
    int held = 0;
    for (int e0 = 0; e0 < k; e0 += 64) {             // (whole waves: the ballot counts the held entries of the previous list)
        const int e = e0 + lane;
        const float v = (accumulate && e < k) ? top_cos[o + e] : -INFINITY;
        const long long i = (accumulate && e < k) ? (long long)top_idx[o + e] : -1LL;
        if (e < k) { rv[e] = v; ri[e] = i; }
        held += __popcll(__ballot(i >= 0));
    }
    __threadfence_block();
    if (lane == 0) { s_thr_v[wave] = rv[k - 1]; s_thr_i[wave] = ri[k - 1]; s_cnt[wave] = held; }
    __threadfence_block();
    for (int s = 0; s < splits; ++s) {
        const long ps = ((long)s * Nq + m) * k;
        for (int e0 = 0; e0 < k; e0 += 64) {
            const int e = e0 + lane;
            const float c = e < k ? pval[ps + e] : -INFINITY;
            const int i = e < k ? pidx[ps + e] : -1;
            const long long gi = idx_offset + i;
            const float tv = s_thr_v[wave];
            const long long ti = s_thr_i[wave];
            const bool live = i >= 0 && (ti < 0 || knn_better<long long>(c, gi, tv, ti));
            const unsigned long long mask = __ballot(live);
            if (!mask) break;
            knn_wave_merge<long long>(rv, ri, k, live, c, gi, mask, lane, s_thr_v + wave, s_thr_i + wave, s_cnt + wave);
            __threadfence_block();                   // the next merge reads what this one wrote
        }
    }
    for (int e = lane; e < k; e += 64) {
        top_cos[o + e] = rv[e];
        top_idx[o + e] = (int64_t)ri[e];
    }
}

// one workgroup per query: the first k threads turn the list into (label or -1, weight); every thread then sums its classes over
// the list in list order
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ top_cos, const int64_t* __restrict__ top_idx, int k,
                                                       const int32_t* __restrict__ base_label, long Nb, int C, float temperature,
                                                       float* __restrict__ scores, int64_t* __restrict__ pred) {
    __shared__ double s_w[CVCL_KNN_MAX_K];
    __shared__ int s_l[CVCL_KNN_MAX_K];
    __shared__ double r_s[256];
    __shared__ int r_c[256];
    const int t = threadIdx.x;
    const long i = blockIdx.x;
    int lab = -1;
    if (t < k) {
        const long idx = (long)top_idx[i * k + t];
        double w = 0.0;
        if (idx >= 0 && idx < Nb) {
            const int l = base_label[idx];
            if (l >= 0 && l < C) {
                lab = l;
                w = temperature > 0.f ? exp((double)top_cos[i * k + t] / (double)temperature) : 1.0;
            }
        }
        s_w[t] = w;
        s_l[t] = lab;
    }
    const int counted = __syncthreads_or(lab >= 0);
    double bs = -1.0;
    int bc = -1;
    for (int c = t; c < C; c += 256) {
        double sum = 0.0;
        for (int j = 0; j < k; ++j)
            if (s_l[j] == c) sum += s_w[j];
        scores[i * C + c] = (float)sum;
        if (sum > bs) { bs = sum; bc = c; }
    }
    r_s[t] = bs;
    r_c[t] = bc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o && r_c[t + o] >= 0 && (r_c[t] < 0 || r_s[t + o] > r_s[t] || (r_s[t + o] == r_s[t] && r_c[t + o] < r_c[t]))) {
            r_s[t] = r_s[t + o];
            r_c[t] = r_c[t + o];
        }
        __syncthreads();
    }
    if (t == 0) pred[i] = counted ? (int64_t)r_c[0] : (int64_t)-1;
}

// ================================================================================================================================
// pixel L1 on 8-bit frames
// ================================================================================================================================
constexpr int PTQ = 8, PTB = 8;                  // frame pairs per wave: PTQ queries x PTB base frames
constexpr int PWAVES = 4;                        // waves per workgroup: PTQ queries x PWAVES * PTB base frames
constexpr int PSETS = PTQ * PTB / 64;            // pair sums per lane after the wave reduction
constexpr int PMAXC = 4;
constexpr int kPixelTargetWgs = 2048;
static_assert(PTQ * PTB % 64 == 0 && 64 % PTB == 0, "a wave's pairs fill whole lane sets; the pairs of one query are adjacent lanes");

struct PixDev {
    const uint8_t* q; const uint8_t* b;
    int Nq, Nb, C, HW;
    double w[PMAXC];
    const int32_t* qg; const int32_t* bg;
    double* pdist; int32_t* pidx; uint32_t* psums;      // [splits][Nq], [splits][Nq], [splits][Nq][C]
    int nbt;                                            // base tiles of PWAVES * PTB frames
    int vec;                                            // frames are 16-byte aligned and HW % 16 == 0
};

__device__ __forceinline__ bool pix_better(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// acc[v] summed over the 64 lanes, the total of acc[set 64 + l] left in lane l (returned per set): at each step a lane keeps one
// half of its values and receives the partner's partial sums of that half
__device__ __forceinline__ void wave_transpose_sum(unsigned (&acc)[PTQ * PTB], unsigned (&out)[PSETS], int lane) {
#pragma unroll
    for (int st = 0; st < PSETS; ++st) {
        unsigned v[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) v[i] = acc[st * 64 + i];
#pragma unroll
        for (int lg = 5; lg >= 0; --lg) {
            const int o = 1 << lg;                   // lane distance = values kept
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int i = 0; i < o; ++i) {
                const unsigned send = up ? v[i] : v[i + o];
                const unsigned keep = up ? v[i + o] : v[i];
                v[i] = keep + (unsigned)__shfl_xor((int)send, o, 64);
            }
        }
        out[st] = v[0];
    }
}

template <int V> struct PixPiece;
template <> struct PixPiece<1> { typedef unsigned type; };
template <> struct PixPiece<4> { typedef u32x4 type; };
__device__ __forceinline__ unsigned piece_get(const unsigned& p, int) { return p; }
__device__ __forceinline__ unsigned piece_get(const u32x4& p, int e) { return p[e]; }

// dwords i0 + lane V, then in steps of 64 V, below i1 of one channel of the wave's PTQ + PTB frames
template <int V>
__device__ __forceinline__ void pix_span(const unsigned* const (&qrow)[PTQ], const unsigned* const (&brow)[PTB], long choff, int i0, int i1,
                                         int lane, unsigned (&acc)[PTQ * PTB]) {
    typedef typename PixPiece<V>::type P;
    for (int i = i0 + lane * V; i < i1; i += 64 * V) {
        P a[PTQ], b[PTB];
#pragma unroll
        for (int x = 0; x < PTQ; ++x) a[x] = *reinterpret_cast<const P*>(qrow[x] + choff + i);
#pragma unroll
        for (int y = 0; y < PTB; ++y) b[y] = *reinterpret_cast<const P*>(brow[y] + choff + i);
#pragma unroll
        for (int e = 0; e < V; ++e)
#pragma unroll
            for (int x = 0; x < PTQ; ++x)
#pragma unroll
                for (int y = 0; y < PTB; ++y)
                    acc[x * PTB + y] = __builtin_amdgcn_sad_u8(piece_get(a[x], e), piece_get(b[y], e), acc[x * PTB + y]);
    }
}

__global__ __launch_bounds__(64 * PWAVES) void nn_l1_u8_kernel(PixDev p) {
    __shared__ double s_d[PWAVES][PTQ];
    __shared__ int s_i[PWAVES][PTQ];
    __shared__ unsigned s_s[PWAVES][PTQ][PMAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * PTQ;
    const int ndw = p.HW / 4;                        // dwords per channel
    const long fdw = (long)p.C * ndw;                // dwords per frame
    const unsigned* qrow[PTQ];
#pragma unroll
    for (int x = 0; x < PTQ; ++x) qrow[x] = reinterpret_cast<const unsigned*>(p.q) + (long)min(q0 + x, p.Nq - 1) * fdw;   // (clamped: masked below)

    // pair v = set 64 + lane of this wave: query v / PTB, base frame v % PTB
    double best_d[PSETS];
    int best_i[PSETS];
    unsigned best_s[PSETS][PMAXC];
    int qg[PSETS];
#pragma unroll
    for (int st = 0; st < PSETS; ++st) {
        best_d[st] = INFINITY; best_i[st] = -1;
#pragma unroll
        for (int c = 0; c < PMAXC; ++c) best_s[st][c] = 0u;
        const int qi = q0 + (st * 64 + lane) / PTB;
        qg[st] = (p.qg && qi < p.Nq) ? p.qg[qi] : 0;
    }
    const int vec_dw = p.vec ? (ndw / 256) * 256 : 0;            // whole 64-lane x 16-byte spans

    for (int bt = blockIdx.y; bt < p.nbt; bt += gridDim.y) {
        const int b0 = (bt * PWAVES + wave) * PTB;
        if (b0 >= p.Nb) continue;                    // (wave-uniform; no barrier inside the loop)
        const unsigned* brow[PTB];
#pragma unroll
        for (int y = 0; y < PTB; ++y) brow[y] = reinterpret_cast<const unsigned*>(p.b) + (long)min(b0 + y, p.Nb - 1) * fdw;
        unsigned sums[PSETS][PMAXC];
#pragma unroll
        for (int st = 0; st < PSETS; ++st)
#pragma unroll
            for (int c = 0; c < PMAXC; ++c) sums[st][c] = 0u;
#pragma unroll
        for (int c = 0; c < PMAXC; ++c) {
            if (c < p.C) {
                unsigned acc[PTQ * PTB];
#pragma unroll
                for (int v = 0; v < PTQ * PTB; ++v) acc[v] = 0u;
                const long choff = (long)c * ndw;
                pix_span<4>(qrow, brow, choff, 0, vec_dw, lane, acc);
                pix_span<1>(qrow, brow, choff, vec_dw, ndw, lane, acc);
                unsigned tot[PSETS];
                wave_transpose_sum(acc, tot, lane);
#pragma unroll
                for (int st = 0; st < PSETS; ++st) sums[st][c] = tot[st];
            }
        }
#pragma unroll
        for (int st = 0; st < PSETS; ++st) {
            const int v = st * 64 + lane;
            const int qi = q0 + v / PTB, bi = b0 + v % PTB;
            double d = (double)sums[st][0] * p.w[0];
#pragma unroll
            for (int c = 1; c < PMAXC; ++c)
                if (c < p.C) d = d + (double)sums[st][c] * p.w[c];
            const bool ok = qi < p.Nq && bi < p.Nb && (!p.bg || p.bg[bi] == qg[st]);
            if (ok && pix_better(d, bi, best_d[st], best_i[st])) {
                best_d[st] = d; best_i[st] = bi;
#pragma unroll
                for (int c = 0; c < PMAXC; ++c) best_s[st][c] = sums[st][c];
            }
        }
    }
    // the PTB lanes of one query, then the workgroup's waves through LDS
#pragma unroll
    for (int st = 0; st < PSETS; ++st) {
#pragma unroll
        for (int o = 1; o < PTB; o <<= 1) {
            const double od = __shfl_xor(best_d[st], o, 64);
            const int oi = __shfl_xor(best_i[st], o, 64);
            unsigned os[PMAXC];
#pragma unroll
            for (int c = 0; c < PMAXC; ++c) os[c] = (unsigned)__shfl_xor((int)best_s[st][c], o, 64);
            if (oi >= 0 && pix_better(od, oi, best_d[st], best_i[st])) {
                best_d[st] = od; best_i[st] = oi;
#pragma unroll
                for (int c = 0; c < PMAXC; ++c) best_s[st][c] = os[c];
            }
        }
        if (lane % PTB == 0) {
            const int x = (st * 64 + lane) / PTB;
            s_d[wave][x] = best_d[st];
            s_i[wave][x] = best_i[st];
#pragma unroll
            for (int c = 0; c < PMAXC; ++c) s_s[wave][x][c] = best_s[st][c];
        }
    }
    __syncthreads();
    const int x = threadIdx.x;
    if (x < PTQ && q0 + x < p.Nq) {
        int bw = 0;
        for (int w = 1; w < PWAVES; ++w)
            if (s_i[w][x] >= 0 && pix_better(s_d[w][x], s_i[w][x], s_d[bw][x], s_i[bw][x])) bw = w;
        const long o = (long)blockIdx.y * p.Nq + q0 + x;
        p.pdist[o] = s_d[bw][x];
        p.pidx[o] = s_i[bw][x];
        for (int c = 0; c < p.C; ++c) p.psums[o * p.C + c] = s_s[bw][x][c];
    }
}

__global__ __launch_bounds__(256) void nn_l1_merge_kernel(const double* __restrict__ pdist, const int32_t* __restrict__ pidx,
                                                          const uint32_t* __restrict__ psums, int splits, int Nq, int C, long idx_offset,
                                                          int accumulate, double* __restrict__ best_dist, int64_t* __restrict__ best_idx,
                                                          uint32_t* __restrict__ best_sums) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nq) return;
    double bd = INFINITY;
    long bi = -1;
    int bs = -1;
    if (accumulate) { bd = best_dist[m]; bi = best_idx[m]; }
    for (int s = 0; s < splits; ++s) {
        const double d = pdist[(long)s * Nq + m];
        const int i = pidx[(long)s * Nq + m];
        if (i < 0) continue;
        const long gi = idx_offset + i;
        if (bi < 0 || d < bd || (d == bd && gi < bi)) { bd = d; bi = gi; bs = s; }
    }
    best_dist[m] = bd;
    best_idx[m] = bi;
    if (best_sums) {
        if (bs >= 0) {
            for (int c = 0; c < C; ++c) best_sums[(long)m * C + c] = psums[((long)bs * Nq + m) * C + c];
        } else if (!accumulate) {
            for (int c = 0; c < C; ++c) best_sums[(long)m * C + c] = 0u;
        }
    }
}

int pixel_splits(int Nq, int Nb) {
    const int qtiles = cvcl_div_up(Nq, PTQ), nbt = cvcl_div_up(Nb, PWAVES * PTB);
    int s = kPixelTargetWgs / qtiles;
    if (s < 1) s = 1;
    return s < nbt ? s : nbt;
}

// ================================================================================================================================
// host side of the cosine searches and the rank count
// ================================================================================================================================
// the workspace: 1 / |row| of both sides (double), then the splits' partial results, `per_query` (value, row) pairs per
// (split, query): 1 for the arg-max, k for the lists.  Byte offsets of 16-byte aligned pieces.
struct CosineWs { size_t invq, invb, pval, pidx, bytes; };

CosineWs cosine_workspace(int Nq, int Nb, int per_query) {
    const size_t nq = align16((size_t)Nq * 8), nb = align16((size_t)Nb * 8);
    const size_t part = align16((size_t)cosine_splits(Nq, Nb) * Nq * per_query * 4);
    return {0, nq, nq + nb, nq + nb + part, nq + nb + 2 * part};
}

// what the three entries share once their arguments are accepted: the walk's arguments, and the two norm passes enqueued
void cosine_begin(CosDev& p, const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps, const int32_t* q_group,
                  const int32_t* base_group, void* workspace, const CosineWs& w, hipStream_t st) {
    char* ws = (char*)workspace;
    double* invq = (double*)(ws + w.invq);
    double* invb = (double*)(ws + w.invb);
    p.q = q; p.b = base; p.ldq = ldq; p.ldb = ldb; p.Nq = Nq; p.Nb = Nb; p.D = D;
    p.invq = invq; p.invb = invb; p.qg = q_group; p.bg = base_group;
    p.pval = (float*)(ws + w.pval); p.pidx = (int32_t*)(ws + w.pidx);
    p.nbt = cvcl_div_up(Nb, CT);
    p.vec = (((uintptr_t)q | (uintptr_t)base) & 15) == 0 && ldq % 4 == 0 && ldb % 4 == 0 && D % 4 == 0;
    nn_inv_norm_kernel<<<cvcl_div_up(Nq, 4), 256, 0, st>>>(q, ldq, Nq, D, eps, invq);
    nn_inv_norm_kernel<<<cvcl_div_up(Nb, 4), 256, 0, st>>>(base, ldb, Nb, D, eps, invb);
}

// cvcl_nn_cosine (topk false; k is not read) and cvcl_knn_cosine (topk true) under the entry's own name and output names
int cosine_search(const char* name, bool topk, const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, int k, float eps,
                  const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, float* out_cos,
                  int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "%s: null pointer (q / base)", name);
    CVCL_CHECK_ARG(out_cos && out_idx, "%s: null pointer (%s)", name, topk ? "top_cos / top_idx" : "best_cos / best_idx");
    CVCL_CHECK_ARG(Nq >= 1, "%s: Nq %d < 1", name, Nq);
    CVCL_CHECK_ARG(Nb >= 1, "%s: Nb %d < 1", name, Nb);
    CVCL_CHECK_ARG(D >= 1, "%s: D %d < 1", name, D);
    CVCL_CHECK_ARG(!topk || (k >= 1 && k <= CVCL_KNN_MAX_K), "%s: k %d outside 1..%d", name, k, CVCL_KNN_MAX_K);
    CVCL_CHECK_ARG(ldq >= D, "%s: ldq %d < D %d", name, ldq, D);
    CVCL_CHECK_ARG(ldb >= D, "%s: ldb %d < D %d", name, ldb, D);
    CVCL_CHECK_ARG(eps >= 0.f, "%s: eps %g < 0", name, (double)eps);
    CVCL_CHECK_ARG((q_group == nullptr) == (base_group == nullptr), "%s: q_group and base_group go together (one is null)", name);
    CVCL_CHECK_ARG(idx_offset >= 0, "%s: idx_offset %lld < 0", name, (long long)idx_offset);
    CVCL_CHECK_ARG(workspace, "%s: null pointer (workspace)", name);
    const CosineWs w = cosine_workspace(Nq, Nb, topk ? k : 1);
    CVCL_CHECK_ARG(workspace_bytes >= w.bytes, "%s: workspace_bytes %zu < %zu", name, workspace_bytes, w.bytes);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", name);

    const int splits = cosine_splits(Nq, Nb);
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_HEAD);
    KnnDev p;
    p.k = k;
    cosine_begin(p, q, ldq, base, ldb, Nq, Nb, D, eps, q_group, base_group, workspace, w, st);
    const dim3 grid(cvcl_div_up(Nq, CT), splits);
    if (topk) {
        if (p.vec) knn_cosine_kernel<true><<<grid, 256, 0, st>>>(p);
        else knn_cosine_kernel<false><<<grid, 256, 0, st>>>(p);
        knn_cosine_merge_kernel<<<cvcl_div_up(Nq, 4), 256, 0, st>>>(p.pval, p.pidx, splits, Nq, k, (long)idx_offset, accumulate, out_cos,
                                                                    out_idx);
    } else {
        if (p.vec) nn_cosine_kernel<true><<<grid, 256, 0, st>>>(p);
        else nn_cosine_kernel<false><<<grid, 256, 0, st>>>(p);
        nn_cosine_merge_kernel<<<cvcl_div_up(Nq, 256), 256, 0, st>>>(p.pval, p.pidx, splits, Nq, (long)idx_offset, accumulate, out_cos,
                                                                     out_idx);
    }
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

}  // namespace

extern "C" size_t cvcl_nn_cosine_workspace_bytes(int Nq, int Nb, int D) {
    if (Nq < 1 || Nb < 1 || D < 1) return 0;
    return cosine_workspace(Nq, Nb, 1).bytes;
}

extern "C" int cvcl_nn_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps,
                              const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, float* best_cos,
                              int64_t* best_idx, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_search("cvcl_nn_cosine", false, q, ldq, base, ldb, Nq, Nb, D, 0, eps, q_group, base_group, idx_offset, accumulate,
                         best_cos, best_idx, workspace, workspace_bytes, stream);
}

extern "C" size_t cvcl_knn_cosine_workspace_bytes(int Nq, int Nb, int D, int k) {
    if (Nq < 1 || Nb < 1 || D < 1 || k < 1 || k > CVCL_KNN_MAX_K) return 0;
    return cosine_workspace(Nq, Nb, k).bytes;
}

extern "C" int cvcl_knn_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, int k, float eps,
                               const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, float* top_cos,
                               int64_t* top_idx, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_search("cvcl_knn_cosine", true, q, ldq, base, ldb, Nq, Nb, D, k, eps, q_group, base_group, idx_offset, accumulate,
                         top_cos, top_idx, workspace, workspace_bytes, stream);
}

extern "C" size_t cvcl_rank_cosine_workspace_bytes(int Nq, int Nb, int D) {
    if (Nq < 1 || Nb < 1 || D < 1) return 0;
    return cosine_workspace(Nq, Nb, 1).bytes;
}

// cvcl_rank_cosine: the arg-max search's workspace layout (its pval piece stays unused), the keys in the group slots
extern "C" int cvcl_rank_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps,
                                const int32_t* q_key, const int32_t* base_key, const float* thr_cos, const int64_t* thr_idx,
                                int64_t idx_offset, int accumulate, int64_t* rank, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "cvcl_rank_cosine: null pointer (q / base)");
    CVCL_CHECK_ARG(q_key && base_key, "cvcl_rank_cosine: null pointer (q_key / base_key)");
    CVCL_CHECK_ARG(thr_cos && thr_idx, "cvcl_rank_cosine: null pointer (thr_cos / thr_idx)");
    CVCL_CHECK_ARG(rank, "cvcl_rank_cosine: null pointer (rank)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_rank_cosine: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_rank_cosine: Nb %d < 1", Nb);
    CVCL_CHECK_ARG(D >= 1, "cvcl_rank_cosine: D %d < 1", D);
    CVCL_CHECK_ARG(ldq >= D, "cvcl_rank_cosine: ldq %d < D %d", ldq, D);
    CVCL_CHECK_ARG(ldb >= D, "cvcl_rank_cosine: ldb %d < D %d", ldb, D);
    CVCL_CHECK_ARG(eps >= 0.f, "cvcl_rank_cosine: eps %g < 0", (double)eps);
    CVCL_CHECK_ARG(idx_offset >= 0, "cvcl_rank_cosine: idx_offset %lld < 0", (long long)idx_offset);
    CVCL_CHECK_ARG(accumulate == 0 || accumulate == 1, "cvcl_rank_cosine: accumulate %d outside {0, 1}", accumulate);
    CVCL_CHECK_ARG(workspace, "cvcl_rank_cosine: null pointer (workspace)");
    const CosineWs w = cosine_workspace(Nq, Nb, 1);
    CVCL_CHECK_ARG(workspace_bytes >= w.bytes, "cvcl_rank_cosine: workspace_bytes %zu < %zu", workspace_bytes, w.bytes);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_rank_cosine: workspace is not 16-byte aligned");

    const int splits = cosine_splits(Nq, Nb);
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_HEAD);
    RankDev p;
    p.thr_cos = thr_cos; p.thr_idx = thr_idx; p.idx_offset = (long)idx_offset;
    cosine_begin(p, q, ldq, base, ldb, Nq, Nb, D, eps, q_key, base_key, workspace, w, st);
    const dim3 grid(cvcl_div_up(Nq, CT), splits);
    if (p.vec) rank_cosine_kernel<true><<<grid, 256, 0, st>>>(p);
    else rank_cosine_kernel<false><<<grid, 256, 0, st>>>(p);
    rank_cosine_merge_kernel<<<cvcl_div_up(Nq, 256), 256, 0, st>>>(p.pidx, splits, Nq, thr_idx, accumulate, rank);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_knn_vote(const float* top_cos, const int64_t* top_idx, int Nq, int k, const int32_t* base_label, int64_t Nb, int C,
                             float temperature, float* scores, int64_t* pred, void* stream) {
    CVCL_CHECK_ARG(top_cos && top_idx, "cvcl_knn_vote: null pointer (top_cos / top_idx)");
    CVCL_CHECK_ARG(base_label, "cvcl_knn_vote: null pointer (base_label)");
    CVCL_CHECK_ARG(scores && pred, "cvcl_knn_vote: null pointer (scores / pred)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_knn_vote: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(k >= 1 && k <= CVCL_KNN_MAX_K, "cvcl_knn_vote: k %d outside 1..%d", k, CVCL_KNN_MAX_K);
    CVCL_CHECK_ARG(C >= 1 && C <= CVCL_KNN_MAX_CLASSES, "cvcl_knn_vote: C %d outside 1..%d", C, CVCL_KNN_MAX_CLASSES);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_knn_vote: Nb %lld < 1", (long long)Nb);
    CVCL_CHECK_ARG(temperature >= 0.f && temperature <= 3.4028234e38f, "cvcl_knn_vote: temperature %g is negative or not finite",
                   (double)temperature);
    CvclProfScope prof(stream, CVCL_K_HEAD);
    knn_vote_kernel<<<Nq, 256, 0, (hipStream_t)stream>>>(top_cos, top_idx, k, base_label, (long)Nb, C, temperature, scores, pred);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" size_t cvcl_nn_l1_u8_workspace_bytes(int Nq, int Nb, int C) {
    if (Nq < 1 || Nb < 1 || C < 1 || C > PMAXC) return 0;
    const size_t s = (size_t)pixel_splits(Nq, Nb);
    return align16(s * Nq * 8) + align16(s * Nq * 4) + align16(s * Nq * C * 4);
}

extern "C" int cvcl_nn_l1_u8(const uint8_t* q, const uint8_t* base, int Nq, int Nb, int C, int HW, const double* w,
                             const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, double* best_dist,
                             int64_t* best_idx, uint32_t* best_sums, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "cvcl_nn_l1_u8: null pointer (q / base)");
    CVCL_CHECK_ARG(w, "cvcl_nn_l1_u8: null pointer (w)");
    CVCL_CHECK_ARG(best_dist && best_idx, "cvcl_nn_l1_u8: null pointer (best_dist / best_idx)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_nn_l1_u8: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_nn_l1_u8: Nb %d < 1", Nb);
    CVCL_CHECK_ARG(C >= 1 && C <= PMAXC, "cvcl_nn_l1_u8: C %d outside 1..%d", C, PMAXC);
    CVCL_CHECK_ARG(HW >= 4 && HW % 4 == 0, "cvcl_nn_l1_u8: HW %d is not a positive multiple of 4", HW);
    CVCL_CHECK_ARG((long long)HW * 255 < (1LL << 32), "cvcl_nn_l1_u8: HW %d: a channel sum can exceed 32 bits", HW);
    CVCL_CHECK_ARG((((uintptr_t)q | (uintptr_t)base) & 3) == 0, "cvcl_nn_l1_u8: q / base are not 4-byte aligned");
    CVCL_CHECK_ARG((q_group == nullptr) == (base_group == nullptr), "cvcl_nn_l1_u8: q_group and base_group go together (one is null)");
    CVCL_CHECK_ARG(idx_offset >= 0, "cvcl_nn_l1_u8: idx_offset %lld < 0", (long long)idx_offset);
    CVCL_CHECK_ARG(workspace, "cvcl_nn_l1_u8: null pointer (workspace)");
    const size_t need = cvcl_nn_l1_u8_workspace_bytes(Nq, Nb, C);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_nn_l1_u8: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_nn_l1_u8: workspace is not 16-byte aligned");

    const int splits = pixel_splits(Nq, Nb);
    char* ws = (char*)workspace;
    PixDev p;
    p.q = q; p.b = base; p.Nq = Nq; p.Nb = Nb; p.C = C; p.HW = HW;
    for (int c = 0; c < PMAXC; ++c) p.w[c] = c < C ? w[c] : 0.0;
    p.qg = q_group; p.bg = base_group;
    p.pdist = (double*)ws; ws += align16((size_t)splits * Nq * 8);
    p.pidx = (int32_t*)ws; ws += align16((size_t)splits * Nq * 4);
    p.psums = (uint32_t*)ws;
    p.nbt = cvcl_div_up(Nb, PWAVES * PTB);
    p.vec = (((uintptr_t)q | (uintptr_t)base) & 15) == 0 && HW % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const dim3 grid(cvcl_div_up(Nq, PTQ), splits);
    nn_l1_u8_kernel<<<grid, 64 * PWAVES, 0, st>>>(p);
    nn_l1_merge_kernel<<<cvcl_div_up(Nq, 256), 256, 0, st>>>(p.pdist, p.pidx, p.psums, splits, Nq, C, (long)idx_offset, accumulate, best_dist,
                                                             best_idx, best_sums);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
