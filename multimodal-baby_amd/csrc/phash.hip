// Perceptual-hash duplicates (gfx950): the 16 x 16 average hash of 8-bit frames and, per evaluation hash, the closest training hash by
// Hamming distance and by the ratio of the hashes written as decimal strings.  Replace, in analysis_cvcl/duplicates.py of the
// reference:
//   :28-41    ahash: cv2.imread(IMREAD_GRAYSCALE) + cv2.resize to 16 x 16 + `resized >= resized.mean()` + the 256-bit integer
//   :333-342  the nested Python loops over every same-category (eval, train) pair with fuzz.ratio(str(eval_hash), str(train_hash))
// Everything here is integer arithmetic (include/cvcl_hip.h "Perceptual-hash duplicates" gives the definitions), so every result is
// exact.  Neither search writes a queries x base matrix, and neither reduces across lanes in its inner loop: a LANE owns one query
// (its hash in registers; its match masks in LDS), the 64 queries of a one-wave workgroup walk a contiguous range of base rows that
// every lane reads at the same address, and the running (best, row) stays in registers.  The ranges' partial results go through
// the caller's workspace to a merge kernel that walks them in ascending order with a strict comparison: no atomics, and ties go to
// the lower index everywhere.
//
// cvcl_ahash_u8        one 256-thread workgroup per frame, one thread per cell: 4 taps x 3 channels = 12 byte loads through the
//                      caller's element strides, the sum of the 256 cells through a wave reduction and LDS, one ballot per wave =
//                      one 64-bit word of the hash.  3 072 bytes of a frame are read, whatever its size: the frame is not streamed.
// cvcl_hamming_nn      4 xor + popcounts per pair; the hashes of 8 base rows are in flight per step (scalar loads).
// cvcl_digit_ratio_nn  bit-parallel LCS, V = (V + (V & M)) | (V & ~M) over two 64-bit words with carry, one step per digit of the
//                      base string.  The per-digit match masks of a lane's query sit in LDS as [digit][lane] 16-byte entries
//                      (conflict-free ds_read_b128); the base strings of a tile, contiguous in memory, are copied to LDS in one
//                      flat pass and read four digits a dword; a lane walks 4 base strings at once (independent chains).
#include "cvcl_common.h"

namespace {

constexpr size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

constexpr int SQ = 64;                           // queries per workgroup of both searches: one wave, a lane per query
constexpr int HAM_MIN_ROWS = 64;                 // base rows per workgroup of the Hamming search, at least
constexpr int RTB = 16;                          // base strings staged per tile of the ratio search
constexpr int RWORDS = CVCL_DIGITS_MAX / 4;      // dwords of a staged base string
constexpr int RIL = 4;                           // base strings a lane walks at once (independent recurrences)
static_assert(RTB % RIL == 0, "a tile is whole groups of interleaved rows");
constexpr int HAM_NONE = 64 * CVCL_AHASH_WORDS + 1;      // the distance of a query without an eligible row: 257
static_assert(CVCL_AHASH_SIDE * CVCL_AHASH_SIDE == 64 * CVCL_AHASH_WORDS && CVCL_AHASH_SIDE * CVCL_AHASH_SIDE == 256,
              "one thread per cell, one wave per word");
static_assert(CVCL_DIGITS_MAX == 128, "the LCS state is two 64-bit words");

// How a search cuts the base rows into contiguous ranges, one per workgroup of a query tile: `rows` a multiple of `unit`, about
// `target` workgroups in all.  Hamming: 2 waves per SIMD on 256 CUs.  Ratio: the search is bound by VALU issue, and with sorted
// groups most (query tile, range) pairs have nothing to do -- short ranges keep the few that do from being the whole kernel's
// critical path (11 workgroups of 13 KiB LDS are resident per CU).
struct SearchShape { int unit, target; };
constexpr SearchShape kHammingShape{HAM_MIN_ROWS, 2048}, kRatioShape{RTB, 8192};
struct BaseSplit { int splits, rows; };
BaseSplit base_split(int Nq, int Nb, SearchShape sh) {
    const int qtiles = cvcl_div_up(Nq, SQ);
    long s = sh.target / qtiles;
    if (s < 1) s = 1;
    long rows = ((long)Nb + s - 1) / s;
    rows = (rows + sh.unit - 1) / sh.unit * sh.unit;
    return {(int)(((long)Nb + rows - 1) / rows), (int)(rows > 0x7fffffffL ? 0x7fffffffL : rows)};
}
size_t search_workspace(int Nq, int Nb, SearchShape sh) {      // [splits][Nq] int32 values, then [splits][Nq] int32 rows
    return 2 * align16((size_t)base_split(Nq, Nb, sh).splits * Nq * 4);
}

// ================================================================================================================================
// average hash
// ================================================================================================================================
__global__ __launch_bounds__(256) void ahash_u8_kernel(const uint8_t* __restrict__ frames, int H, int W, long sn, long sc, long sy, long sx,
                                                       int64_t* __restrict__ hash, int32_t* __restrict__ cells) {
    __shared__ int s_sum[CVCL_AHASH_WORDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cy = t / CVCL_AHASH_SIDE, cx = t % CVCL_AHASH_SIDE;
    // sample position ((2 d + 1) n - 16) / 32 on each axis; the clamp of the second tap is reached at n = 16 only, where w1 = 0
    const long numy = (long)(2 * cy + 1) * H - 16, numx = (long)(2 * cx + 1) * W - 16;
    const long y0 = numy >> 5, x0 = numx >> 5;
    const int wy1 = (int)(numy & 31), wx1 = (int)(numx & 31), wy0 = 32 - wy1, wx0 = 32 - wx1;
    const long y1 = y0 + 1 < H ? y0 + 1 : (long)H - 1, x1 = x0 + 1 < W ? x0 + 1 : (long)W - 1;
    const uint8_t* f = frames + (long)blockIdx.x * sn;
    auto grey = [&](long y, long x) {
        const uint8_t* p = f + y * sy + x * sx;
        return (19595 * (int)p[0] + 38470 * (int)p[sc] + 7471 * (int)p[2 * sc] + 32768) >> 16;
    };
    const int g00 = grey(y0, x0), g01 = grey(y0, x1), g10 = grey(y1, x0), g11 = grey(y1, x1);
    const int v = wy0 * (wx0 * g00 + wx1 * g01) + wy1 * (wx0 * g10 + wx1 * g11);        // scaled by 1024
    const int r = (v + 512) >> 10;
    if (cells) cells[(long)blockIdx.x * 256 + t] = r;
    int s = r;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_sum[wave] = s;
    __syncthreads();
    const int total = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const unsigned long long word = __ballot(256 * r >= total);      // bit 16 y + x = t: lane l of wave w is bit 64 w + l
    if (lane == 0) hash[(long)blockIdx.x * CVCL_AHASH_WORDS + wave] = (int64_t)word;
}

// ================================================================================================================================
// Hamming
// ================================================================================================================================
// HAM_UNROLL base rows per step: their 32-byte hashes (and groups) are read at wave-uniform addresses before any is used, so a step
// waits for one round trip of the loads, not one per row
constexpr int HAM_UNROLL = 8;

template <bool GROUPED>
__global__ __launch_bounds__(SQ) void hamming_nn_kernel(const unsigned long long* __restrict__ q, const unsigned long long* __restrict__ base,
                                                        int Nq, int Nb, int rows, const int32_t* __restrict__ qg,
                                                        const int32_t* __restrict__ bg, int32_t* __restrict__ pdist,
                                                        int32_t* __restrict__ pidx) {
    const int m = blockIdx.x * SQ + threadIdx.x;
    const long mc = m < Nq ? m : Nq - 1;             // (clamped: not written below)
    const unsigned long long q0 = q[4 * mc], q1 = q[4 * mc + 1], q2 = q[4 * mc + 2], q3 = q[4 * mc + 3];
    const int g = GROUPED ? qg[mc] : 0;
    const long j0 = (long)blockIdx.y * rows;
    const int j1 = (int)(j0 + rows < Nb ? j0 + rows : (long)Nb);
    int bd = HAM_NONE, bi = -1;
    auto pair = [&](int j, const unsigned long long (&b)[4], int gb) {
        const int d = __popcll(q0 ^ b[0]) + __popcll(q1 ^ b[1]) + __popcll(q2 ^ b[2]) + __popcll(q3 ^ b[3]);
        const bool take = (!GROUPED || gb == g) && d < bd;       // (strict: the lower row keeps a tie)
        bd = take ? d : bd;
        bi = take ? j : bi;
    };
    int j = (int)j0;
    for (; j + HAM_UNROLL <= j1; j += HAM_UNROLL) {  // (every lane reads the same addresses)
        unsigned long long b[HAM_UNROLL][4];
        int gb[HAM_UNROLL];
#pragma unroll
        for (int u = 0; u < HAM_UNROLL; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) b[u][w] = base[4 * (long)(j + u) + w];
            gb[u] = GROUPED ? bg[j + u] : 0;
        }
#pragma unroll
        for (int u = 0; u < HAM_UNROLL; ++u) pair(j + u, b[u], gb[u]);
    }
    for (; j < j1; ++j) {
        const unsigned long long b[4] = {base[4 * (long)j], base[4 * (long)j + 1], base[4 * (long)j + 2], base[4 * (long)j + 3]};
        pair(j, b, GROUPED ? bg[j] : 0);
    }
    if (m < Nq) {
        pdist[(long)blockIdx.y * Nq + m] = bd;
        pidx[(long)blockIdx.y * Nq + m] = bi;
    }
}

// the splits' partials in ascending order of their rows; LOWER is the Hamming search (the minimum), otherwise the maximum
template <bool LOWER>
__global__ __launch_bounds__(256) void hash_merge_kernel(const int32_t* __restrict__ pval, const int32_t* __restrict__ pidx, int splits, int Nq,
                                                         int none, int32_t* __restrict__ best_val, int64_t* __restrict__ best_idx) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nq) return;
    int bv = none;
    long bi = -1;
    for (int s = 0; s < splits; ++s) {
        const int v = pval[(long)s * Nq + m], i = pidx[(long)s * Nq + m];
        if (i >= 0 && (LOWER ? v < bv : v > bv)) { bv = v; bi = i; }
    }
    best_val[m] = bv;
    best_idx[m] = bi;
}

// ================================================================================================================================
// ratio of digit strings
// ================================================================================================================================
// VEC: ld % 4 == 0 and base is 4-byte aligned -- a tile of base strings is copied and read by dwords, otherwise by bytes
template <bool VEC>
__global__ __launch_bounds__(SQ) void digit_ratio_nn_kernel(const uint8_t* __restrict__ q, const int32_t* __restrict__ q_len,
                                                            const uint8_t* __restrict__ base, const int32_t* __restrict__ base_len, int Nq,
                                                            int Nb, int ld, int rows, const int32_t* __restrict__ qg,
                                                            const int32_t* __restrict__ bg, int32_t* __restrict__ pratio,
                                                            int32_t* __restrict__ pidx) {
    __shared__ __attribute__((aligned(16))) unsigned long long sM[11][SQ][2];       // match masks; row 10: a byte above 9 matches nothing
    __shared__ __attribute__((aligned(16))) unsigned sB[RTB * RWORDS];               // the tile's rows as they lie, ld bytes apart
    __shared__ int sL[RTB], sG[RTB];
    const int lane = threadIdx.x;
    const int m = blockIdx.x * SQ + lane;
    const bool valid = m < Nq;
    const long mc = m < Nq ? m : Nq - 1;
    const int la = valid ? min(max(q_len[mc], 0), ld) : 0;
    const int g = qg ? qg[mc] : 0;
#pragma unroll
    for (int d = 0; d < 11; ++d) { sM[d][lane][0] = 0ull; sM[d][lane][1] = 0ull; }
    for (int k = 0; k < la; ++k) {                   // (a lane touches its own entries only)
        const int c = q[mc * ld + k];
        if (c < 10) sM[c][lane][k >> 6] |= 1ull << (k & 63);
    }
    // the low la bits
    const unsigned long long mlo = la >= 64 ? ~0ull : (1ull << la) - 1ull;
    const unsigned long long mhi = la <= 64 ? 0ull : (la >= 128 ? ~0ull : (1ull << (la - 64)) - 1ull);

    const long j0 = (long)blockIdx.y * rows;
    const long j1 = j0 + rows < Nb ? j0 + rows : (long)Nb;
    int br = 0, bi = -1;
    for (long t0 = j0; t0 < j1; t0 += RTB) {
        __syncthreads();                             // the previous tile is read
        // the tile's rows are contiguous: one flat copy whose loads are all in flight together, and one lane per row for its
        // length and group (a row beyond the range gets length 0)
        const int nrows = (int)(j1 - t0 < RTB ? j1 - t0 : (long)RTB);
        if (lane < RTB) {
            const bool row_ok = lane < nrows;
            sL[lane] = row_ok ? min(max(base_len[t0 + lane], 0), ld) : 0;
            sG[lane] = (bg && row_ok) ? bg[t0 + lane] : 0;
        }
        const uint8_t* src = base + t0 * ld;
        if (VEC) {
            const unsigned* src4 = reinterpret_cast<const unsigned*>(src);
            const int ndw = nrows * ld / 4;
#pragma unroll
            for (int u = 0; u < RTB * RWORDS / SQ; ++u)
                if (lane + SQ * u < ndw) sB[lane + SQ * u] = src4[lane + SQ * u];
        } else {
            uint8_t* dst = reinterpret_cast<uint8_t*>(sB);
            const int nbytes = nrows * ld;
#pragma unroll
            for (int u = 0; u < RTB * CVCL_DIGITS_MAX / SQ; ++u)
                if (lane + SQ * u < nbytes) dst[lane + SQ * u] = src[lane + SQ * u];
        }
        __syncthreads();
        // RIL rows at a time: their recurrences are independent chains (LDS read of the mask, two 64-bit adds with carry), and a
        // lone chain leaves the wave waiting for its own latency at every digit
        for (int s0 = 0; s0 < RTB; s0 += RIL) {
            int lb[RIL], lmax = 0;
            bool elig[RIL];
#pragma unroll
            for (int r = 0; r < RIL; ++r) {
                elig[r] = la > 0 && (!bg || sG[s0 + r] == g);
                lb[r] = __ballot(elig[r]) ? sL[s0 + r] : 0;          // (wave-uniform; a row no lane may take is not walked)
                lmax = max(lmax, lb[r]);
            }
            if (lmax <= 0) continue;
            unsigned long long vlo[RIL], vhi[RIL];
#pragma unroll
            for (int r = 0; r < RIL; ++r) { vlo[r] = ~0ull; vhi[r] = ~0ull; }
            for (int k4 = 0; 4 * k4 < lmax; ++k4) {
                // four digits of each row; bytes behind a string's length (the next row, or what an earlier tile left) are not used
                unsigned w[RIL];
#pragma unroll
                for (int r = 0; r < RIL; ++r) {
                    if (VEC) {
                        w[r] = sB[(s0 + r) * ld / 4 + k4];
                    } else {
                        const uint8_t* row = reinterpret_cast<const uint8_t*>(sB) + (s0 + r) * ld + 4 * k4;
                        w[r] = (unsigned)row[0] | ((unsigned)row[1] << 8) | ((unsigned)row[2] << 16) | ((unsigned)row[3] << 24);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int r = 0; r < RIL; ++r) {
                        if (4 * k4 + e < lb[r]) {                    // (wave-uniform)
                            const int c = min((int)((w[r] >> (8 * e)) & 255u), 10);
                            const unsigned long long Mlo = sM[c][lane][0], Mhi = sM[c][lane][1];
                            const unsigned long long slo = vlo[r] + (vlo[r] & Mlo);
                            const unsigned long long carry = slo < vlo[r] ? 1ull : 0ull;
                            const unsigned long long shi = vhi[r] + (vhi[r] & Mhi) + carry;
                            vlo[r] = slo | (vlo[r] & ~Mlo);
                            vhi[r] = shi | (vhi[r] & ~Mhi);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RIL; ++r) {                          // (in row order: the lower row keeps a tie)
                if (lb[r] <= 0) continue;
                const int lcs = la - __popcll(vlo[r] & mlo) - __popcll(vhi[r] & mhi);
                // round_half_even(200 lcs / (la + lb)) by quotient and remainder
                const unsigned den = (unsigned)(la + lb[r]), num = 200u * (unsigned)lcs;
                const unsigned qv = num / den, rem = num - qv * den;
                const int ratio = (int)(qv + ((2u * rem > den || (2u * rem == den && (qv & 1u))) ? 1u : 0u));
                if (elig[r] && ratio > br) { br = ratio; bi = (int)(t0 + s0 + r); }
            }
        }
    }
    if (valid) {
        pratio[(long)blockIdx.y * Nq + m] = br;
        pidx[(long)blockIdx.y * Nq + m] = bi;
    }
}

}  // namespace

extern "C" int cvcl_ahash_u8(const uint8_t* frames, int N, int H, int W, long stride_n, long stride_c, long stride_y, long stride_x,
                             int64_t* hash, int32_t* cells, void* stream) {
    CVCL_CHECK_ARG(frames, "cvcl_ahash_u8: null pointer (frames)");
    CVCL_CHECK_ARG(hash, "cvcl_ahash_u8: null pointer (hash)");
    CVCL_CHECK_ARG(N >= 1, "cvcl_ahash_u8: N %d < 1", N);
    CVCL_CHECK_ARG(H >= CVCL_AHASH_SIDE, "cvcl_ahash_u8: H %d < %d", H, CVCL_AHASH_SIDE);
    CVCL_CHECK_ARG(W >= CVCL_AHASH_SIDE, "cvcl_ahash_u8: W %d < %d", W, CVCL_AHASH_SIDE);
    CVCL_CHECK_ARG(stride_n >= 1, "cvcl_ahash_u8: stride_n %ld < 1", stride_n);
    CVCL_CHECK_ARG(stride_c >= 1, "cvcl_ahash_u8: stride_c %ld < 1", stride_c);
    CVCL_CHECK_ARG(stride_y >= 1, "cvcl_ahash_u8: stride_y %ld < 1", stride_y);
    CVCL_CHECK_ARG(stride_x >= 1, "cvcl_ahash_u8: stride_x %ld < 1", stride_x);
    CvclProfScope prof(stream, CVCL_K_OTHER);
    ahash_u8_kernel<<<N, 256, 0, (hipStream_t)stream>>>(frames, H, W, stride_n, stride_c, stride_y, stride_x, hash, cells);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" size_t cvcl_hamming_nn_workspace_bytes(int Nq, int Nb) {
    if (Nq < 1 || Nb < 1) return 0;
    return search_workspace(Nq, Nb, kHammingShape);
}

extern "C" int cvcl_hamming_nn(const int64_t* q, const int64_t* base, int Nq, int Nb, const int32_t* q_group, const int32_t* base_group,
                               int32_t* best_dist, int64_t* best_idx, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "cvcl_hamming_nn: null pointer (q / base)");
    CVCL_CHECK_ARG(best_dist && best_idx, "cvcl_hamming_nn: null pointer (best_dist / best_idx)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_hamming_nn: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_hamming_nn: Nb %d < 1", Nb);
    CVCL_CHECK_ARG((q_group == nullptr) == (base_group == nullptr), "cvcl_hamming_nn: q_group and base_group go together (one is null)");
    CVCL_CHECK_ARG(workspace, "cvcl_hamming_nn: null pointer (workspace)");
    const size_t need = search_workspace(Nq, Nb, kHammingShape);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_hamming_nn: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_hamming_nn: workspace is not 16-byte aligned");

    const BaseSplit sp = base_split(Nq, Nb, kHammingShape);
    int32_t* pdist = (int32_t*)workspace;
    int32_t* pidx = (int32_t*)((char*)workspace + need / 2);
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const dim3 grid(cvcl_div_up(Nq, SQ), sp.splits);
    const unsigned long long* uq = (const unsigned long long*)q;
    const unsigned long long* ub = (const unsigned long long*)base;
    if (q_group) hamming_nn_kernel<true><<<grid, SQ, 0, st>>>(uq, ub, Nq, Nb, sp.rows, q_group, base_group, pdist, pidx);
    else hamming_nn_kernel<false><<<grid, SQ, 0, st>>>(uq, ub, Nq, Nb, sp.rows, q_group, base_group, pdist, pidx);
    hash_merge_kernel<true><<<cvcl_div_up(Nq, 256), 256, 0, st>>>(pdist, pidx, sp.splits, Nq, HAM_NONE, best_dist, best_idx);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" size_t cvcl_digit_ratio_nn_workspace_bytes(int Nq, int Nb) {
    if (Nq < 1 || Nb < 1) return 0;
    return search_workspace(Nq, Nb, kRatioShape);
}

extern "C" int cvcl_digit_ratio_nn(const uint8_t* q, const int32_t* q_len, const uint8_t* base, const int32_t* base_len, int Nq, int Nb,
                                   int ld, const int32_t* q_group, const int32_t* base_group, int32_t* best_ratio, int64_t* best_idx,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(q && base, "cvcl_digit_ratio_nn: null pointer (q / base)");
    CVCL_CHECK_ARG(q_len && base_len, "cvcl_digit_ratio_nn: null pointer (q_len / base_len)");
    CVCL_CHECK_ARG(best_ratio && best_idx, "cvcl_digit_ratio_nn: null pointer (best_ratio / best_idx)");
    CVCL_CHECK_ARG(Nq >= 1, "cvcl_digit_ratio_nn: Nq %d < 1", Nq);
    CVCL_CHECK_ARG(Nb >= 1, "cvcl_digit_ratio_nn: Nb %d < 1", Nb);
    CVCL_CHECK_ARG(ld >= 1 && ld <= CVCL_DIGITS_MAX, "cvcl_digit_ratio_nn: ld %d outside 1..%d", ld, CVCL_DIGITS_MAX);
    CVCL_CHECK_ARG((q_group == nullptr) == (base_group == nullptr),
                   "cvcl_digit_ratio_nn: q_group and base_group go together (one is null)");
    CVCL_CHECK_ARG(workspace, "cvcl_digit_ratio_nn: null pointer (workspace)");
    const size_t need = search_workspace(Nq, Nb, kRatioShape);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_digit_ratio_nn: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_digit_ratio_nn: workspace is not 16-byte aligned");

    const BaseSplit sp = base_split(Nq, Nb, kRatioShape);
    int32_t* pratio = (int32_t*)workspace;
    int32_t* pidx = (int32_t*)((char*)workspace + need / 2);
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const dim3 grid(cvcl_div_up(Nq, SQ), sp.splits);
    if (ld % 4 == 0 && ((uintptr_t)base & 3) == 0)
        digit_ratio_nn_kernel<true><<<grid, SQ, 0, st>>>(q, q_len, base, base_len, Nq, Nb, ld, sp.rows, q_group, base_group, pratio, pidx);
    else
        digit_ratio_nn_kernel<false><<<grid, SQ, 0, st>>>(q, q_len, base, base_len, Nq, Nb, ld, sp.rows, q_group, base_group, pratio, pidx);
    hash_merge_kernel<false><<<cvcl_div_up(Nq, 256), 256, 0, st>>>(pratio, pidx, sp.splits, Nq, 0, best_ratio, best_idx);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
