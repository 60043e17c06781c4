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

__device__ __forceinline__ bool cos_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

template <bool VEC>
__global__ __launch_bounds__(256, 2) void nn_cosine_kernel(CosDev p) {
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
    float best_v[2] = {-INFINITY, -INFINITY};
    int best_i[2] = {-1, -1};
    double invq[2];
    int qg[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + wm * 64 + mt * 32 + l31;
        invq[mt] = m < p.Nq ? p.invq[m] : 0.0;
        qg[mt] = (p.qg && m < p.Nq) ? p.qg[m] : 0;
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
            __syncthreads();                         // the previous step's fragments are read
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
                    if (n_ok && g == qg[mt] && cos_better(c, n, best_v[mt], best_i[mt])) { best_v[mt] = c; best_i[mt] = n; }
                }
            }
    }
    // lane halves, then the two waves of a query half (through LDS), then one partial per query and split
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const float ov = __shfl_xor(best_v[mt], 32, 64);
        const int oi = __shfl_xor(best_i[mt], 32, 64);
        if (oi >= 0 && cos_better(ov, oi, best_v[mt], best_i[mt])) { best_v[mt] = ov; best_i[mt] = oi; }
    }
    __syncthreads();
    float* rv = reinterpret_cast<float*>(smem);                  // [2][128]
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
        if (i1 >= 0 && cos_better(v1, i1, v, i)) { v = v1; i = i1; }
        p.pval[(long)blockIdx.y * p.Nq + m0 + tid] = v;
        p.pidx[(long)blockIdx.y * p.Nq + m0 + tid] = i;
    }
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

}  // namespace

extern "C" size_t cvcl_nn_cosine_workspace_bytes(int Nq, int Nb, int D) {
    if (Nq < 1 || Nb < 1 || D < 1) return 0;
    const size_t s = (size_t)cosine_splits(Nq, Nb);
    return align16((size_t)Nq * 8) + align16((size_t)Nb * 8) + align16(s * Nq * 4) + align16(s * Nq * 4);
}

extern "C" int cvcl_nn_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps,
                              const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, float* best_cos,
                              int64_t* best_idx, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "cvcl_nn_cosine: null pointer (q / base)");
    CVCL_CHECK_ARG(best_cos && best_idx, "cvcl_nn_cosine: null pointer (best_cos / best_idx)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_nn_cosine: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_nn_cosine: Nb %d < 1", Nb);
    CVCL_CHECK_ARG(D >= 1, "cvcl_nn_cosine: D %d < 1", D);
    CVCL_CHECK_ARG(ldq >= D, "cvcl_nn_cosine: ldq %d < D %d", ldq, D);
    CVCL_CHECK_ARG(ldb >= D, "cvcl_nn_cosine: ldb %d < D %d", ldb, D);
    CVCL_CHECK_ARG(eps >= 0.f, "cvcl_nn_cosine: eps %g < 0", (double)eps);
    CVCL_CHECK_ARG((q_group == nullptr) == (base_group == nullptr), "cvcl_nn_cosine: q_group and base_group go together (one is null)");
    CVCL_CHECK_ARG(idx_offset >= 0, "cvcl_nn_cosine: idx_offset %lld < 0", (long long)idx_offset);
    CVCL_CHECK_ARG(workspace, "cvcl_nn_cosine: null pointer (workspace)");
    const size_t need = cvcl_nn_cosine_workspace_bytes(Nq, Nb, D);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_nn_cosine: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_nn_cosine: workspace is not 16-byte aligned");

    const int splits = cosine_splits(Nq, Nb);
    char* ws = (char*)workspace;
    CosDev p;
    p.q = q; p.b = base; p.ldq = ldq; p.ldb = ldb; p.Nq = Nq; p.Nb = Nb; p.D = D;
    double* invq = (double*)ws; ws += align16((size_t)Nq * 8);
    double* invb = (double*)ws; ws += align16((size_t)Nb * 8);
    p.pval = (float*)ws; ws += align16((size_t)splits * Nq * 4);
    p.pidx = (int32_t*)ws;
    p.invq = invq; p.invb = invb; p.qg = q_group; p.bg = base_group;
    p.nbt = cvcl_div_up(Nb, CT);
    p.vec = (((uintptr_t)q | (uintptr_t)base) & 15) == 0 && ldq % 4 == 0 && ldb % 4 == 0 && D % 4 == 0;
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_HEAD);
    nn_inv_norm_kernel<<<cvcl_div_up(Nq, 4), 256, 0, st>>>(q, ldq, Nq, D, eps, invq);
    nn_inv_norm_kernel<<<cvcl_div_up(Nb, 4), 256, 0, st>>>(base, ldb, Nb, D, eps, invb);
    const dim3 grid(cvcl_div_up(Nq, CT), splits);
    if (p.vec) nn_cosine_kernel<true><<<grid, 256, 0, st>>>(p);
    else nn_cosine_kernel<false><<<grid, 256, 0, st>>>(p);
    nn_cosine_merge_kernel<<<cvcl_div_up(Nq, 256), 256, 0, st>>>(p.pval, p.pidx, splits, Nq, (long)idx_offset, accumulate, best_cos, best_idx);
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
