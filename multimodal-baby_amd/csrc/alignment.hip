// Image-text alignment analysis (gfx950): per-class mean features, cosine matrices, Pearson correlation of two strict upper
// triangles and paired Euclidean distances.  Replace the per-element torch / numpy loops of the reference:
//   analysis_cvcl/alignment.py:106-110    np.mean over the frames of each category                     -> cvcl_class_mean_f32
//   analysis_cvcl/alignment.py:148-161, :182-195 and analysis_tools/representation_similarity.py:5-12
//                                         F.cosine_similarity(F.normalize(a_i), F.normalize(b_j)) per pair -> cvcl_cosine_matrix_f32
//   analysis_cvcl/alignment.py:230-232 and representation_similarity.py:30-39
//                                         scipy.stats.pearsonr of the two np.triu_indices(k=1) selections   -> cvcl_triu_pearson_f32
//   analysis_cvcl/embeddings.py:106-111   F.pairwise_distance(x_i, y_i, p=2) per category                   -> cvcl_paired_l2_f32
// All fp32 in, sums in double (products of the cosine matrix: exact fp32 MFMA, chains added in double), no floating-point atomics:
// every summation order is a function of the shapes and the labels alone, so two calls give the same bits.
//
// cvcl_class_mean_f32     a stable counting sort of the row indices by label (per-chunk histograms with LDS integer counters, a
//                         column scan over the chunks, one wave per chunk that ranks its rows in order), then one workgroup per
//                         (class, 128 columns): 8 row streams of 32 lanes x 16 bytes, 4 rows in flight each, double accumulators,
//                         merged in a fixed order.  Classes may be of any size; rows need not be grouped.
// cvcl_cosine_matrix_f32  T x T outputs per 256-thread workgroup (T = 16 while that fills the chip, 32 otherwise), the four waves
//                         take interleaved k steps of the SAME tile (a 22 x 22 matrix at D = 512 is 4 workgroups of 4 waves with 8
//                         loads each, not one long chain); operands go from global memory straight into the MFMA (each lane 16
//                         bytes of one row), the squared norms are summed in double from the same registers.  a == b: tiles below
//                         the diagonal are skipped and every element is written to (i, j) and (j, i): symmetric by construction.
// cvcl_triu_pearson_f32   each workgroup takes rows i, i + G, ...: means of its share, then centred second moments about them
//                         (both in double), one partial per workgroup; one wave merges the partials pairwise in a fixed tree
//                         (Chan et al.) and forms r.  A side whose minimum equals its maximum gives r = NaN (scipy's constant input).
#include "cvcl_common.h"

namespace {

constexpr size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

constexpr int kMaxD = 2048, kMaxClasses = 4096, kMaxN = 1 << 24, kMaxRows = 4096;

// ================================================================================================================================
// class means
// ================================================================================================================================
constexpr int kMaxChunks = 256;          // histogram rows
constexpr int kMeanCols = 128;           // columns per workgroup of the mean kernel
constexpr int kMeanStreams = 8;          // row streams per workgroup (4 waves x 2 half-waves)
constexpr int kMeanUnroll = 4;           // rows in flight per stream

struct ChunkPlan { int rows, n; };
ChunkPlan chunk_plan(int N) {
    int rows = cvcl_div_up(N, kMaxChunks);
    rows = cvcl_div_up(rows, 64) * 64;
    if (rows < 256) rows = 256;
    return {rows, cvcl_div_up(N, rows)};
}

// hist[chunk][c] = rows of class c in the chunk (integer LDS counters: exact, order-free)
__global__ __launch_bounds__(256) void cm_hist_kernel(const int32_t* __restrict__ label, int N, int C, int chunk_rows,
                                                      int32_t* __restrict__ hist) {
    __shared__ int cnt[kMaxClasses];
    for (int c = threadIdx.x; c < C; c += 256) cnt[c] = 0;
    __syncthreads();
    const int r0 = blockIdx.x * chunk_rows, r1 = min(N, r0 + chunk_rows);
    for (int r = r0 + threadIdx.x; r < r1; r += 256) {
        const int l = label[r];
        if ((unsigned)l < (unsigned)C) atomicAdd(&cnt[l], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) hist[(long)blockIdx.x * C + c] = cnt[c];
}

// per class: hist[.][c] -> exclusive prefix over the chunks, count[c] = total
__global__ __launch_bounds__(256) void cm_scan_chunks_kernel(int32_t* __restrict__ hist, int nchunks, int C, int32_t* __restrict__ count) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int run = 0;
    for (int k = 0; k < nchunks; ++k) {
        const int t = hist[(long)k * C + c];
        hist[(long)k * C + c] = run;
        run += t;
    }
    count[c] = run;
}

// class_off[c] = sum of count[< c] (one workgroup; C <= 4096 = 256 threads x 16)
__global__ __launch_bounds__(256) void cm_offsets_kernel(const int32_t* __restrict__ count, int C, int32_t* __restrict__ class_off) {
    __shared__ int part[256];
    const int per = (C + 255) / 256, c0 = threadIdx.x * per;
    int s = 0;
    for (int i = 0; i < per; ++i)
        if (c0 + i < C) s += count[c0 + i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = 0; i < per; ++i)
        if (c0 + i < C) { class_off[c0 + i] = run; run += count[c0 + i]; }
}

// one wave per chunk: perm[class_off[l] + rows of class l before r] = r, rows in ascending order inside every class
__global__ __launch_bounds__(64) void cm_scatter_kernel(const int32_t* __restrict__ label, int N, int C, int chunk_rows,
                                                        const int32_t* __restrict__ hist, const int32_t* __restrict__ class_off,
                                                        int32_t* __restrict__ perm) {
    __shared__ int base[kMaxClasses];
    const int lane = threadIdx.x;
    for (int c = lane; c < C; c += 64) base[c] = class_off[c] + hist[(long)blockIdx.x * C + c];
    __syncthreads();
    const int r0 = blockIdx.x * chunk_rows, r1 = min(N, r0 + chunk_rows);
    for (int s = r0; s < r1; s += 64) {                // (wave-uniform bounds: every lane runs every step)
        const int r = s + lane;
        int l = r < r1 ? label[r] : -1;
        if ((unsigned)l >= (unsigned)C) l = -1;
        int before = 0, total = 0;
        for (int j = 0; j < 64; ++j) {
            const int lj = __shfl(l, j, 64);
            before += (lj == l && j < lane) ? 1 : 0;
            total += (lj == l) ? 1 : 0;
        }
        if (l >= 0) perm[base[l] + before] = r;
        __syncthreads();
        if (l >= 0 && before == total - 1) base[l] += total;       // the last row of each label in this step, alone
        __syncthreads();
    }
}

// 16 bytes (or 4 guarded scalars) of row r at column col
__device__ __forceinline__ f32x4 load4(const float* __restrict__ x, long r, int D, int col, bool vec) {
    const float* p = x + r * D + col;
    if (vec) return col < D ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = col + e < D ? p[e] : 0.f;
    return v;
}

__global__ __launch_bounds__(256) void cm_mean_kernel(const float* __restrict__ x, int D, const int32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ class_off, const int32_t* __restrict__ count, int vec,
                                                      float* __restrict__ mean) {
    __shared__ double part[kMeanStreams][kMeanCols];
    const int c = blockIdx.x, col = blockIdx.y * kMeanCols + (threadIdx.x & 31) * 4, stream = threadIdx.x >> 5;
    const int n = count[c];
    const int32_t* members = perm + class_off[c];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = stream; m0 < n; m0 += kMeanStreams * kMeanUnroll) {
        f32x4 v[kMeanUnroll];
#pragma unroll
        for (int u = 0; u < kMeanUnroll; ++u) {
            const int m = m0 + u * kMeanStreams;
            v[u] = m < n ? load4(x, (long)members[m], D, col, vec != 0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < kMeanUnroll; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (double)v[u][e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[stream][(threadIdx.x & 31) * 4 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < kMeanCols) {
        const int oc = blockIdx.y * kMeanCols + threadIdx.x;
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kMeanStreams; ++k) s += part[k][threadIdx.x];
        if (oc < D) mean[(long)c * D + oc] = n > 0 ? (float)(s / (double)n) : 0.f;
    }
}

// ================================================================================================================================
// cosine matrix
// ================================================================================================================================
template <int T> struct Mfma;
template <> struct Mfma<32> {                      // v_mfma_f32_32x32x2_f32: lane = row (l & 31), k half (l >> 5)
    typedef f32x16 Acc;
    static constexpr int kGroups = 2, kAcc = 16;
    __device__ static __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    __device__ static __forceinline__ int arow(int e, int g) { return 8 * (e >> 2) + 4 * g + (e & 3); }
};
template <> struct Mfma<16> {                      // v_mfma_f32_16x16x4_f32: lane = row (l & 15), k quarter (l >> 4)
    typedef f32x4 Acc;
    static constexpr int kGroups = 4, kAcc = 4;
    __device__ static __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static __forceinline__ int arow(int e, int g) { return 4 * g + e; }
};

template <int T>
__global__ __launch_bounds__(256) void cosine_matrix_kernel(const float* __restrict__ a, const float* __restrict__ b, int M, int K, int D,
                                                            float eps, int vec, int same, float* __restrict__ out) {
    typedef Mfma<T> MM;
    constexpr int G = MM::kGroups, STEP = 4 * G;            // k per wave step: every lane holds 4 consecutive k of its group
    constexpr int UN = 4;
    __shared__ float s_dot[4][T][T + 1];
    __shared__ double s_na[4][G][T], s_nb[4][G][T];
    __shared__ double s_ia[T], s_ib[T];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (same && tj < ti) return;                            // (workgroup-uniform) the mirror of tile (tj, ti) covers it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & (T - 1), g = lane / T;
    const int ia = ti * T + row, ib = tj * T + row;
    const long ra = min(ia, M - 1), rb = min(ib, K - 1);    // clamped: rows beyond the matrix are computed and not written
    typename MM::Acc acc;
#pragma unroll
    for (int e = 0; e < MM::kAcc; ++e) acc[e] = 0.f;
    double na = 0.0, nb = 0.0;
    const int steps = (D + STEP - 1) / STEP;
    for (int s0 = wave; s0 < steps; s0 += 4 * UN) {
        f32x4 fa[UN], fb[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = s0 + 4 * u;
            const int col = s < steps ? s * STEP + 4 * g : D;     // beyond the last step: zeros
            fa[u] = load4(a, ra, D, col, vec != 0);
            fb[u] = load4(b, rb, D, col, vec != 0);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc = MM::mma(fa[u][e], fb[u][e], acc);
                na += (double)fa[u][e] * (double)fa[u][e];
                nb += (double)fb[u][e] * (double)fb[u][e];
            }
    }
#pragma unroll
    for (int e = 0; e < MM::kAcc; ++e) s_dot[wave][MM::arow(e, g)][row] = acc[e];
    s_na[wave][g][row] = na;
    s_nb[wave][g][row] = nb;
    __syncthreads();
    if (tid < 2 * T) {
        const int r = tid & (T - 1);
        double s = 0.0;
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < G; ++q) s += tid < T ? s_na[w][q][r] : s_nb[w][q][r];
        const double inv = 1.0 / fmax(sqrt(s), (double)eps);
        if (tid < T) s_ia[r] = inv; else s_ib[r] = inv;
    }
    __syncthreads();
    for (int idx = tid; idx < T * T; idx += 256) {
        const int i = idx / T, j = idx % T;
        const int gi = ti * T + i, gj = tj * T + j;
        if (gi >= M || gj >= K) continue;
        if (same && gj < gi) continue;                      // (diagonal tile) written by its mirror
        const double dot = (((double)s_dot[0][i][j] + (double)s_dot[1][i][j]) + (double)s_dot[2][i][j]) + (double)s_dot[3][i][j];
        const float v = (float)(dot * (s_ia[i] * s_ib[j]));
        out[(long)gi * K + gj] = v;
        if (same && gj != gi) out[(long)gj * K + gi] = v;
    }
}

// ================================================================================================================================
// Pearson correlation of two strict upper triangles
// ================================================================================================================================
constexpr int kPearsonMaxWgs = 256;
struct Moments { double n, ma, mb, qa, qb, qab, lo_a, hi_a, lo_b, hi_b; };      // counts, means, centred sums, extremes
constexpr int kMomentDoubles = 10;

// x then y (the order matters to the last bit: every merge below names the lower-numbered partial first)
__device__ __forceinline__ Moments merge(const Moments& x, const Moments& y) {
    if (y.n == 0.0) return x;
    if (x.n == 0.0) return y;
    Moments r;
    r.n = x.n + y.n;
    const double da = y.ma - x.ma, db = y.mb - x.mb, f = x.n * y.n / r.n;
    r.ma = x.ma + da * (y.n / r.n);
    r.mb = x.mb + db * (y.n / r.n);
    r.qa = (x.qa + y.qa) + da * da * f;
    r.qb = (x.qb + y.qb) + db * db * f;
    r.qab = (x.qab + y.qab) + da * db * f;
    r.lo_a = fmin(x.lo_a, y.lo_a); r.hi_a = fmax(x.hi_a, y.hi_a);
    r.lo_b = fmin(x.lo_b, y.lo_b); r.hi_b = fmax(x.hi_b, y.hi_b);
    return r;
}

// sum over the 256 threads, the same value in every thread (xor tree per wave, then the four waves in order)
__device__ __forceinline__ double block_sum_f64(double v, double* scratch) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

__global__ __launch_bounds__(256) void pearson_partial_kernel(const float* __restrict__ A, const float* __restrict__ B, int C,
                                                              double* __restrict__ partials) {
    __shared__ double scratch[4];
    const int tid = threadIdx.x;
    double sa = 0.0, sb = 0.0, cnt = 0.0;
    double lo_a = INFINITY, hi_a = -INFINITY, lo_b = INFINITY, hi_b = -INFINITY;
    for (int i = blockIdx.x; i < C - 1; i += gridDim.x) {
        const float* ra = A + (long)i * C;
        const float* rb = B + (long)i * C;
        for (int j = i + 1 + tid; j < C; j += 256) {
            const double va = (double)ra[j], vb = (double)rb[j];
            sa += va; sb += vb; cnt += 1.0;
            lo_a = fmin(lo_a, va); hi_a = fmax(hi_a, va);
            lo_b = fmin(lo_b, vb); hi_b = fmax(hi_b, vb);
        }
    }
    const double n = block_sum_f64(cnt, scratch);
    const double ma = n > 0.0 ? block_sum_f64(sa, scratch) / n : 0.0;
    const double mb = n > 0.0 ? block_sum_f64(sb, scratch) / n : 0.0;
    double qa = 0.0, qb = 0.0, qab = 0.0;
    for (int i = blockIdx.x; i < C - 1; i += gridDim.x) {
        const float* ra = A + (long)i * C;
        const float* rb = B + (long)i * C;
        for (int j = i + 1 + tid; j < C; j += 256) {
            const double da = (double)ra[j] - ma, db = (double)rb[j] - mb;
            qa += da * da; qb += db * db; qab += da * db;
        }
    }
    qa = block_sum_f64(qa, scratch);
    qb = block_sum_f64(qb, scratch);
    qab = block_sum_f64(qab, scratch);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_a = fmin(lo_a, __shfl_xor(lo_a, o, 64)); hi_a = fmax(hi_a, __shfl_xor(hi_a, o, 64));
        lo_b = fmin(lo_b, __shfl_xor(lo_b, o, 64)); hi_b = fmax(hi_b, __shfl_xor(hi_b, o, 64));
    }
    __shared__ double ext[4][4];
    if ((tid & 63) == 0) { ext[tid >> 6][0] = lo_a; ext[tid >> 6][1] = hi_a; ext[tid >> 6][2] = lo_b; ext[tid >> 6][3] = hi_b; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            lo_a = fmin(lo_a, ext[w][0]); hi_a = fmax(hi_a, ext[w][1]);
            lo_b = fmin(lo_b, ext[w][2]); hi_b = fmax(hi_b, ext[w][3]);
        }
        double* p = partials + (long)blockIdx.x * kMomentDoubles;
        p[0] = n; p[1] = ma; p[2] = mb; p[3] = qa; p[4] = qb; p[5] = qab; p[6] = lo_a; p[7] = hi_a; p[8] = lo_b; p[9] = hi_b;
    }
}

__device__ __forceinline__ Moments shfl_xor_moments(const Moments& m, int o) {
    Moments r;
    r.n = __shfl_xor(m.n, o, 64); r.ma = __shfl_xor(m.ma, o, 64); r.mb = __shfl_xor(m.mb, o, 64);
    r.qa = __shfl_xor(m.qa, o, 64); r.qb = __shfl_xor(m.qb, o, 64); r.qab = __shfl_xor(m.qab, o, 64);
    r.lo_a = __shfl_xor(m.lo_a, o, 64); r.hi_a = __shfl_xor(m.hi_a, o, 64);
    r.lo_b = __shfl_xor(m.lo_b, o, 64); r.hi_b = __shfl_xor(m.hi_b, o, 64);
    return r;
}

// one wave: lane l folds partials l, l + 64, ... in ascending order, then a fixed xor tree (the lower lane's value first)
__global__ __launch_bounds__(64) void pearson_merge_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ out6) {
    const int lane = threadIdx.x;
    Moments m;
    m.n = m.ma = m.mb = m.qa = m.qb = m.qab = 0.0;
    m.lo_a = m.lo_b = INFINITY; m.hi_a = m.hi_b = -INFINITY;
    for (int k = lane; k < nparts; k += 64) {
        const double* p = partials + (long)k * kMomentDoubles;
        Moments y;
        y.n = p[0]; y.ma = p[1]; y.mb = p[2]; y.qa = p[3]; y.qb = p[4]; y.qab = p[5]; y.lo_a = p[6]; y.hi_a = p[7]; y.lo_b = p[8]; y.hi_b = p[9];
        m = merge(m, y);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Moments other = shfl_xor_moments(m, o);
        m = (lane & o) ? merge(other, m) : merge(m, other);
    }
    if (lane == 0) {
        double r = __builtin_nan("");
        if (m.lo_a < m.hi_a && m.lo_b < m.hi_b && m.qa > 0.0 && m.qb > 0.0) {
            r = m.qab / (sqrt(m.qa) * sqrt(m.qb));
            r = fmax(-1.0, fmin(1.0, r));
        }
        out6[0] = m.n; out6[1] = r; out6[2] = m.ma; out6[3] = m.mb; out6[4] = m.qa / m.n; out6[5] = m.qb / m.n;
    }
}

int pearson_wgs(int C) { return C - 1 < kPearsonMaxWgs ? C - 1 : kPearsonMaxWgs; }

// ================================================================================================================================
// paired distances: one wave per row
// ================================================================================================================================
__global__ __launch_bounds__(256) void paired_l2_kernel(const float* __restrict__ x, const float* __restrict__ y, int C, int D, float eps,
                                                        float* __restrict__ d) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= C) return;                                   // (wave-uniform)
    const float* xr = x + (long)row * D;
    const float* yr = y + (long)row * D;
    double s = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double t = ((double)xr[k] - (double)yr[k]) + (double)eps;
        s += t * t;
    }
    s = wave_sum(s);
    if (lane == 0) d[row] = (float)sqrt(s);
}

}  // namespace

extern "C" size_t cvcl_class_mean_workspace_bytes(int N, int D, int C) {
    if (N < 1 || N >= kMaxN || D < 1 || D > kMaxD || C < 1 || C > kMaxClasses) return 0;
    const ChunkPlan cp = chunk_plan(N);
    return align16((size_t)cp.n * C * 4) + align16((size_t)C * 4) + align16((size_t)N * 4);
}

extern "C" int cvcl_class_mean_f32(const float* x, const int32_t* label, int N, int D, int C, float* mean, int32_t* count, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(x && label, "cvcl_class_mean_f32: null pointer (x / label)");
    CVCL_CHECK_ARG(mean && count, "cvcl_class_mean_f32: null pointer (mean / count)");
    CVCL_CHECK_ARG(N >= 1, "cvcl_class_mean_f32: N %d < 1", N);
    CVCL_CHECK_ARG(N < kMaxN, "cvcl_class_mean_f32: N %d >= 2^24", N);
    CVCL_CHECK_ARG(D >= 1 && D <= kMaxD, "cvcl_class_mean_f32: D %d outside 1..%d", D, kMaxD);
    CVCL_CHECK_ARG(C >= 1 && C <= kMaxClasses, "cvcl_class_mean_f32: C %d outside 1..%d", C, kMaxClasses);
    CVCL_CHECK_ARG(workspace, "cvcl_class_mean_f32: null pointer (workspace)");
    const size_t need = cvcl_class_mean_workspace_bytes(N, D, C);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_class_mean_f32: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "cvcl_class_mean_f32: workspace is not 16-byte aligned");

    const ChunkPlan cp = chunk_plan(N);
    char* ws = (char*)workspace;
    int32_t* hist = (int32_t*)ws; ws += align16((size_t)cp.n * C * 4);
    int32_t* class_off = (int32_t*)ws; ws += align16((size_t)C * 4);
    int32_t* perm = (int32_t*)ws;
    const int vec = ((uintptr_t)x & 15) == 0 && D % 4 == 0;
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    cm_hist_kernel<<<cp.n, 256, 0, st>>>(label, N, C, cp.rows, hist);
    cm_scan_chunks_kernel<<<cvcl_div_up(C, 256), 256, 0, st>>>(hist, cp.n, C, count);
    cm_offsets_kernel<<<1, 256, 0, st>>>(count, C, class_off);
    cm_scatter_kernel<<<cp.n, 64, 0, st>>>(label, N, C, cp.rows, hist, class_off, perm);
    cm_mean_kernel<<<dim3(C, cvcl_div_up(D, kMeanCols)), 256, 0, st>>>(x, D, perm, class_off, count, vec, mean);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_cosine_matrix_f32(const float* a, const float* b, int M, int K, int D, float eps, float* out, void* stream) {
    CVCL_CHECK_ARG(a && b, "cvcl_cosine_matrix_f32: null pointer (a / b)");
    CVCL_CHECK_ARG(out, "cvcl_cosine_matrix_f32: null pointer (out)");
    CVCL_CHECK_ARG(M >= 1 && M <= kMaxRows, "cvcl_cosine_matrix_f32: M %d outside 1..%d", M, kMaxRows);
    CVCL_CHECK_ARG(K >= 1 && K <= kMaxRows, "cvcl_cosine_matrix_f32: K %d outside 1..%d", K, kMaxRows);
    CVCL_CHECK_ARG(D >= 1 && D <= kMaxD, "cvcl_cosine_matrix_f32: D %d outside 1..%d", D, kMaxD);
    CVCL_CHECK_ARG(eps >= 0.f, "cvcl_cosine_matrix_f32: eps %g < 0", (double)eps);
    CVCL_CHECK_ARG(a != b || M == K, "cvcl_cosine_matrix_f32: a == b needs M == K (got %d, %d)", M, K);

    const int vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && D % 4 == 0;
    const int same = a == b;
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_HEAD);
    // 16 x 16 tiles while 32 x 32 ones would leave compute units without a workgroup (256 of them)
    if ((long)cvcl_div_up(M, 32) * cvcl_div_up(K, 32) < 256)
        cosine_matrix_kernel<16><<<dim3(cvcl_div_up(K, 16), cvcl_div_up(M, 16)), 256, 0, st>>>(a, b, M, K, D, eps, vec, same, out);
    else
        cosine_matrix_kernel<32><<<dim3(cvcl_div_up(K, 32), cvcl_div_up(M, 32)), 256, 0, st>>>(a, b, M, K, D, eps, vec, same, out);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" size_t cvcl_triu_pearson_workspace_bytes(int C) {
    if (C < 3 || C > kMaxRows) return 0;
    return align16((size_t)pearson_wgs(C) * kMomentDoubles * 8);
}

extern "C" int cvcl_triu_pearson_f32(const float* A, const float* B, int C, double* out6, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    CVCL_CHECK_ARG(A && B, "cvcl_triu_pearson_f32: null pointer (A / B)");
    CVCL_CHECK_ARG(out6, "cvcl_triu_pearson_f32: null pointer (out)");
    CVCL_CHECK_ARG(C >= 3, "cvcl_triu_pearson_f32: C %d < 3", C);
    CVCL_CHECK_ARG(C <= kMaxRows, "cvcl_triu_pearson_f32: C %d > %d", C, kMaxRows);
    CVCL_CHECK_ARG(workspace, "cvcl_triu_pearson_f32: null pointer (workspace)");
    const size_t need = cvcl_triu_pearson_workspace_bytes(C);
    CVCL_CHECK_ARG(workspace_bytes >= need, "cvcl_triu_pearson_f32: workspace_bytes %zu < %zu", workspace_bytes, need);
    CVCL_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out6 & 7) == 0, "cvcl_triu_pearson_f32: workspace / out are not aligned");

    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const int wgs = pearson_wgs(C);
    pearson_partial_kernel<<<wgs, 256, 0, st>>>(A, B, C, (double*)workspace);
    pearson_merge_kernel<<<1, 64, 0, st>>>((const double*)workspace, wgs, out6);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_paired_l2_f32(const float* x, const float* y, int C, int D, float eps, float* d, void* stream) {
    CVCL_CHECK_ARG(x && y, "cvcl_paired_l2_f32: null pointer (x / y)");
    CVCL_CHECK_ARG(d, "cvcl_paired_l2_f32: null pointer (d)");
    CVCL_CHECK_ARG(C >= 1 && C <= kMaxClasses, "cvcl_paired_l2_f32: C %d outside 1..%d", C, kMaxClasses);
    CVCL_CHECK_ARG(D >= 1 && D <= kMaxD, "cvcl_paired_l2_f32: D %d outside 1..%d", D, kMaxD);
    hipStream_t st = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
    paired_l2_kernel<<<cvcl_div_up(C, 4), 256, 0, st>>>(x, y, C, D, eps, d);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
