// Map faithfulness (cvcl_hip.h "Map faithfulness"): the deletion / insertion curves of an attention map (Petsiuk et al., RISE, 2018).
// The pixels of a frame are removed (or, from a blurred frame, restored) in the order the map ranks them, the frame is re-encoded
// after every slice, and the areas under the two score curves say how faithful the map is (multimodal/map_faithfulness.py).
//
// Kernels: map_ranks_kernel (one workgroup per map: a stable LSD radix sort of (monotone key, 16-bit pixel index) pairs, 8 bits per
// pass, ping-pong in the caller's scratch; the last pass scatters the ranks themselves), map_perturb_kernel (a pure select of
// image / baseline by rank < count, up to PT_ITEMS work items per launch, their (map, image, count, mode) in the argument block),
// blur_axis_kernel (one axis of the separable reflect-padded Gaussian, weights in the argument block), pair_dot_kernel (one wave per
// row), curve_auc_kernel (one thread per curve).  No atomics on global memory: two calls give the same bits.
#include <math.h>

#include "cvcl_common.h"

namespace {

constexpr int RK_MAX_HW = 65536;                      // pixel indices travel as 16 bits
constexpr int RK_THREADS = 1024, RK_WAVES = RK_THREADS / 64;
constexpr int RK_BINS = 256, RK_PASSES = 4;           // 8-bit digits of the 32-bit key
constexpr int PT_ITEMS = 256;                         // work items of one map_perturb_kernel launch (3 KiB of the argument block)
constexpr int PT_PX = 4;                              // pixels per thread
constexpr int BL_MAX_K = 129;                         // taps of the Gaussian

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// Keys that sort ascending as the values sort descending: the usual monotone map of the float bits (negative: all bits flipped,
// else the sign bit set), complemented.  -0.0 is read as +0.0 first; subnormals keep their bits, so they order by value.
__device__ __forceinline__ unsigned rank_key(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

// One workgroup sorts map blockIdx.x.  hist[p][d]: how many keys have digit d in pass p (one read of the map, before the passes: a
// histogram does not depend on the order).  A pass whose keys all share one digit moves nothing and is left out.  Each remaining pass
// walks its input in tiles of RK_THREADS elements in index order; inside a tile a lane's place among the lanes of its wave with the
// same digit comes from 8 ballots, the waves' counts per digit are scanned in wave order, and base[d] runs on from tile to tile: the
// scatter is stable, so equal keys stay in pixel order and ties go to the lower flat index.  The first pass reads the map itself, the
// last one writes ranks[index] = position instead of the pair.
__global__ __launch_bounds__(RK_THREADS) void map_ranks_kernel(const float* __restrict__ maps, int32_t* __restrict__ ranks, int HW,
                                                               unsigned* key_buf, unsigned short* idx_buf, long key_stride,
                                                               long idx_stride) {
    __shared__ unsigned hist[RK_PASSES][RK_BINS];
    __shared__ unsigned base[RK_BINS];
    __shared__ unsigned wave_cnt[RK_WAVES][RK_BINS];
    __shared__ int active[RK_PASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src_map = maps + (long)blockIdx.x * HW;
    int32_t* dst_rank = ranks + (long)blockIdx.x * HW;
    unsigned* kb[2] = {key_buf + (long)blockIdx.x * 2 * key_stride, key_buf + ((long)blockIdx.x * 2 + 1) * key_stride};
    unsigned short* ib[2] = {idx_buf + (long)blockIdx.x * 2 * idx_stride, idx_buf + ((long)blockIdx.x * 2 + 1) * idx_stride};

    for (int i = tid; i < RK_PASSES * RK_BINS; i += RK_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (int i = tid; i < HW; i += RK_THREADS) {
        const unsigned k = rank_key(src_map[i]);
#pragma unroll
        for (int p = 0; p < RK_PASSES; ++p) atomicAdd(&hist[p][(k >> (8 * p)) & 0xffu], 1u);
    }
    __syncthreads();
    if (tid < RK_PASSES) {                            // exclusive scan of pass tid's histogram, in place
        unsigned run = 0u;
        int moves = 1;
        for (int d = 0; d < RK_BINS; ++d) {
            const unsigned c = hist[tid][d];
            if (c == (unsigned)HW) moves = 0;
            hist[tid][d] = run;
            run += c;
        }
        active[tid] = moves;
    }
    __syncthreads();
    int last = -1;
    for (int p = 0; p < RK_PASSES; ++p)
        if (active[p]) last = p;
    if (last < 0) {                                   // all keys equal: the order is the pixel order
        for (int i = tid; i < HW; i += RK_THREADS) dst_rank[i] = i;
        return;
    }
    bool from_map = true;
    int cur = 0;                                      // the buffer the next pass reads (once from_map is false)
    for (int p = 0; p <= last; ++p) {
        if (!active[p]) continue;                     // (uniform: active[] is shared)
        if (tid < RK_BINS) base[tid] = hist[p][tid];
        const unsigned* kin = kb[cur];
        const unsigned short* iin = ib[cur];
        unsigned* kout = kb[cur ^ 1];
        unsigned short* iout = ib[cur ^ 1];
        for (int s = 0; s < HW; s += RK_THREADS) {
            for (int i = tid; i < RK_WAVES * RK_BINS; i += RK_THREADS) (&wave_cnt[0][0])[i] = 0u;
            __syncthreads();                          // (also: base[] of this pass / of the previous tile is written)
            const int i = s + tid;
            const bool valid = i < HW;
            unsigned k = 0u, idx = 0u;
            if (valid) {
                if (from_map) { k = rank_key(src_map[i]); idx = (unsigned)i; }
                else { k = kin[i]; idx = iin[i]; }
            }
            const unsigned d = (k >> (8 * p)) & 0xffu;
            unsigned long long peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const unsigned long long m = __ballot(valid && ((d >> b) & 1u));
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            const unsigned before = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
            if (valid && before == 0u) wave_cnt[wave][d] = (unsigned)__popcll(peers);
            __syncthreads();
            if (tid < RK_BINS) {                      // digit tid: the waves' counts become their first positions
                unsigned run = base[tid];
#pragma unroll
                for (int w = 0; w < RK_WAVES; ++w) {
                    const unsigned c = wave_cnt[w][tid];
                    wave_cnt[w][tid] = run;
                    run += c;
                }
                base[tid] = run;
            }
            __syncthreads();
            if (valid) {
                const unsigned pos = wave_cnt[wave][d] + before;          // < HW: the histogram counted exactly these keys
                if (p == last) dst_rank[idx] = (int32_t)pos;
                else { kout[pos] = k; iout[pos] = (unsigned short)idx; }
            }
            __syncthreads();                          // wave_cnt is zeroed next
        }
        // the next pass reads what this one wrote: other threads' global stores, ordered by the tile's last barrier (workgroup scope)
        from_map = false;
        cur ^= 1;
    }
}

struct PtItem { int map, image, count_mode; };       // count_mode: count | mode << 30
struct PtArgs {
    const float* images; const float* baseline; const int32_t* ranks;
    float* out;
    int C, HW, vec;
    PtItem item[PT_ITEMS];
};

// out[item][c][p] = (ranks[map][p] < count) == (mode == 0) ? baseline[image][c][p] : images[image][c][p]; a NULL baseline is zeros
__global__ __launch_bounds__(256) void map_perturb_kernel(PtArgs a, int tiles) {
    const int item = blockIdx.x / tiles, tile = blockIdx.x - item * tiles;
    const PtItem it = a.item[item];
    const int count = it.count_mode & 0x3fffffff, insertion = it.count_mode >> 30;
    const int HW = a.HW, C = a.C;
    const long p = ((long)tile * 256 + threadIdx.x) * PT_PX;
    if (p >= HW) return;
    const int32_t* rk = a.ranks + (long)it.map * HW + p;
    const float* img = a.images + (long)it.image * C * HW + p;
    const float* bas = a.baseline ? a.baseline + (long)it.image * C * HW + p : nullptr;
    float* out = a.out + (long)item * C * HW + p;
    if (a.vec) {
        const int4 r = *reinterpret_cast<const int4*>(rk);
        const bool t0 = (r.x < count) != (insertion != 0), t1 = (r.y < count) != (insertion != 0);
        const bool t2 = (r.z < count) != (insertion != 0), t3 = (r.w < count) != (insertion != 0);      // true: the baseline's value
        for (int c = 0; c < C; ++c) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(img + (long)c * HW);
            const f32x4 b = bas ? *reinterpret_cast<const f32x4*>(bas + (long)c * HW) : f32x4{0.f, 0.f, 0.f, 0.f};
            stream_store(f32x4{t0 ? b[0] : x[0], t1 ? b[1] : x[1], t2 ? b[2] : x[2], t3 ? b[3] : x[3]},
                         reinterpret_cast<f32x4*>(out + (long)c * HW));
        }
    } else {
        const int n = min((long)PT_PX, HW - p);
        for (int q = 0; q < n; ++q) {
            const bool take_base = (rk[q] < count) != (insertion != 0);
            for (int c = 0; c < C; ++c) out[(long)c * HW + q] = take_base ? (bas ? bas[(long)c * HW + q] : 0.f) : img[(long)c * HW + q];
        }
    }
}

struct BlurW { float w[BL_MAX_K]; };

// torch's "reflect" (c b | a b c d | c b): the edge is not repeated; one reflection is enough for a radius below n
__device__ __forceinline__ int reflect_no_edge(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }

// AXIS 1: along a row (x), AXIS 0: along a column (y); taps added in index order
template <int AXIS>
__global__ __launch_bounds__(256) void blur_axis_kernel(const float* __restrict__ in, float* __restrict__ out, BlurW w, int k, long total,
                                                        int H, int W) {
    const int r = k / 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / W;
        const int x = (int)(e - row * W);
        const long plane = row / H;
        const int y = (int)(row - plane * H);
        const float* src = in + plane * H * W;
        float acc = 0.f;
        for (int t = 0; t < k; ++t) {
            const float v = AXIS == 1 ? src[(long)y * W + reflect_no_edge(x - r + t, W)] : src[(long)reflect_no_edge(y - r + t, H) * W + x];
            acc = fmaf(w.w[t], v, acc);
        }
        out[e] = acc;
    }
}

// out[r] = <rows[r], targets[target_of_row[r]]>: one wave per row, lane l adds elements l, l + 64, ... in order, then the wave sum
__global__ __launch_bounds__(256) void pair_dot_kernel(const float* __restrict__ rows, const float* __restrict__ targets,
                                                       const int32_t* __restrict__ target_of_row, float* __restrict__ out, int R, int M,
                                                       int E) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int t = target_of_row[r];
    if (t < 0 || t >= M) {                            // an index outside the targets: no access, NaN
        if (lane == 0) out[r] = __builtin_nanf("");
        return;
    }
    const float* a = rows + r * E;
    const float* b = targets + (long)t * E;
    float acc = 0.f;
    for (int e = lane; e < E; e += 64) acc = fmaf(a[e], b[e], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[r] = acc;
}

// auc[k][m] = sum_s (x[s + 1] - x[s]) (y[k][s][m] + y[k][s + 1][m]) / 2
__global__ __launch_bounds__(256) void curve_auc_kernel(const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ auc,
                                                        int K, int S, int M) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)K * M) return;
    const long k = e / M, m = e - k * M;
    const float* yk = y + k * (S + 1) * M + m;
    float acc = 0.f, prev = yk[0];
    for (int s = 0; s < S; ++s) {
        const float next = yk[(long)(s + 1) * M];
        acc = fmaf(x[s + 1] - x[s], 0.5f * (prev + next), acc);
        prev = next;
    }
    auc[e] = acc;
}

inline size_t rank_key_bytes(int HW) { return round16((size_t)HW * sizeof(unsigned)); }
inline size_t rank_idx_bytes(int HW) { return round16((size_t)HW * sizeof(unsigned short)); }

}  // namespace

extern "C" size_t cvcl_map_ranks_scratch_bytes(int M, int HW) {
    if (M < 1 || HW < 1 || HW > RK_MAX_HW) return 0;
    return (size_t)M * 2 * (rank_key_bytes(HW) + rank_idx_bytes(HW));
}

extern "C" int cvcl_map_ranks(const float* maps, int32_t* ranks, int M, int HW, void* scratch, size_t scratch_bytes, void* stream) {
    CVCL_CHECK_ARG(maps && ranks, "cvcl_map_ranks: null pointer (maps / ranks)");
    CVCL_CHECK_ARG(M >= 1, "cvcl_map_ranks: M %d < 1", M);
    CVCL_CHECK_ARG(HW >= 1 && HW <= RK_MAX_HW, "cvcl_map_ranks: HW %d is outside 1 .. %d", HW, RK_MAX_HW);
    CVCL_CHECK_ARG(scratch, "cvcl_map_ranks: null pointer (scratch)");
    const size_t need = cvcl_map_ranks_scratch_bytes(M, HW);
    CVCL_CHECK_ARG(scratch_bytes >= need, "cvcl_map_ranks: scratch_bytes %zu < %zu needed", scratch_bytes, need);
    CVCL_CHECK_ARG(cvcl_aligned16(scratch), "cvcl_map_ranks: scratch is not 16-byte aligned");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    unsigned* keys = (unsigned*)scratch;
    unsigned short* idx = (unsigned short*)((char*)scratch + (size_t)M * 2 * rank_key_bytes(HW));
    hipLaunchKernelGGL(map_ranks_kernel, dim3((unsigned)M), dim3(RK_THREADS), 0, (hipStream_t)stream, maps, ranks, HW, keys, idx,
                       (long)(rank_key_bytes(HW) / sizeof(unsigned)), (long)(rank_idx_bytes(HW) / sizeof(unsigned short)));
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_map_perturb(const float* images, const float* baseline, const int32_t* ranks, const int32_t* image_of_map,
                                const int32_t* item_map, const int32_t* item_count, const int32_t* item_mode, int n_items, int N, int M,
                                int C, int H, int W, float* out, void* stream) {
    CVCL_CHECK_ARG(images && ranks && out, "cvcl_map_perturb: null pointer (images / ranks / out)");
    CVCL_CHECK_ARG(item_map && item_count && item_mode, "cvcl_map_perturb: null pointer (item_map / item_count / item_mode)");
    CVCL_CHECK_ARG(n_items >= 1 && N >= 1 && M >= 1 && C >= 1, "cvcl_map_perturb: n_items %d, N %d, M %d, C %d must be positive", n_items, N, M, C);
    CVCL_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= RK_MAX_HW, "cvcl_map_perturb: H x W = %d x %d is outside 1 .. %d pixels", H, W, RK_MAX_HW);
    CVCL_CHECK_ARG(image_of_map || M <= N, "cvcl_map_perturb: without image_of_map map m lies over image m, but M %d > N %d", M, N);
    const int HW = H * W;
    for (int m = 0; image_of_map && m < M; ++m)
        CVCL_CHECK_ARG(image_of_map[m] >= 0 && image_of_map[m] < N, "cvcl_map_perturb: image_of_map[%d] = %d is outside 0 .. %d", m,
                       image_of_map[m], N - 1);
    for (int i = 0; i < n_items; ++i) {
        CVCL_CHECK_ARG(item_map[i] >= 0 && item_map[i] < M, "cvcl_map_perturb: item_map[%d] = %d is outside 0 .. %d", i, item_map[i], M - 1);
        CVCL_CHECK_ARG(item_count[i] >= 0 && item_count[i] <= HW, "cvcl_map_perturb: item_count[%d] = %d is outside 0 .. %d", i, item_count[i], HW);
        CVCL_CHECK_ARG(item_mode[i] == 0 || item_mode[i] == 1, "cvcl_map_perturb: item_mode[%d] = %d outside {0, 1}", i, item_mode[i]);
    }
    const int tiles = cvcl_div_up(HW, 256 * PT_PX);
    CvclProfScope prof(stream, CVCL_K_OTHER);
    PtArgs a;
    a.images = images; a.baseline = baseline; a.ranks = ranks;
    a.C = C; a.HW = HW;
    a.vec = (HW % PT_PX == 0) && cvcl_aligned16(images) && cvcl_aligned16(baseline) && cvcl_aligned16(ranks) && cvcl_aligned16(out);
    for (int s = 0; s < n_items; s += PT_ITEMS) {
        const int n = n_items - s < PT_ITEMS ? n_items - s : PT_ITEMS;
        for (int i = 0; i < n; ++i) {
            const int m = item_map[s + i];
            a.item[i].map = m;
            a.item[i].image = image_of_map ? image_of_map[m] : m;
            a.item[i].count_mode = item_count[s + i] | (item_mode[s + i] << 30);
        }
        a.out = out + (size_t)s * C * HW;
        hipLaunchKernelGGL(map_perturb_kernel, dim3((unsigned)((long)n * tiles)), dim3(256), 0, (hipStream_t)stream, a, tiles);
        CVCL_LAUNCH_CHECK();
    }
    return CVCL_OK;
}

extern "C" int cvcl_gaussian_blur_f32(const float* x, float* y, const float* w, int k, int planes, int H, int W, void* scratch,
                                      void* stream) {
    CVCL_CHECK_ARG(x && y && w && scratch, "cvcl_gaussian_blur_f32: null pointer (x / y / w / scratch)");
    CVCL_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1, "cvcl_gaussian_blur_f32: planes %d, H %d, W %d must be positive", planes, H, W);
    CVCL_CHECK_ARG(k >= 1 && (k & 1), "cvcl_gaussian_blur_f32: k %d is not a positive odd number", k);
    CVCL_CHECK_ARG(k <= BL_MAX_K, "cvcl_gaussian_blur_f32: k %d > %d", k, BL_MAX_K);
    CVCL_CHECK_ARG(k / 2 < (H < W ? H : W), "cvcl_gaussian_blur_f32: the radius k / 2 = %d does not lie below min(H, W) = %d (reflect padding)",
                   k / 2, H < W ? H : W);
    CVCL_CHECK_ARG(x != y && (const void*)x != scratch && (void*)y != scratch, "cvcl_gaussian_blur_f32: x, y and scratch must be distinct");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    BlurW bw;
    for (int t = 0; t < BL_MAX_K; ++t) bw.w[t] = t < k ? w[t] : 0.f;
    const long total = (long)planes * H * W;
    const int grid = cvcl_grid(total, 256, 8192);
    hipLaunchKernelGGL(blur_axis_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (float*)scratch, bw, k, total, H, W);
    CVCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(blur_axis_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, y, bw, k, total, H, W);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_pair_dot(const float* rows, const float* targets, const int32_t* target_of_row, float* out, int R, int M, int E,
                             void* stream) {
    CVCL_CHECK_ARG(rows && targets && target_of_row && out, "cvcl_pair_dot: null pointer (rows / targets / target_of_row / out)");
    CVCL_CHECK_ARG(R >= 1 && M >= 1 && E >= 1, "cvcl_pair_dot: R %d, M %d, E %d must be positive", R, M, E);
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(pair_dot_kernel, dim3((unsigned)cvcl_div_up(R, 4)), dim3(256), 0, (hipStream_t)stream, rows, targets, target_of_row,
                       out, R, M, E);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_curve_auc(const float* y, const float* x, float* auc, int K, int S, int M, void* stream) {
    CVCL_CHECK_ARG(y && x && auc, "cvcl_curve_auc: null pointer (y / x / auc)");
    CVCL_CHECK_ARG(K >= 1 && S >= 1 && M >= 1, "cvcl_curve_auc: K %d, S %d, M %d must be positive", K, S, M);
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(curve_auc_kernel, dim3((unsigned)cvcl_div_up((long)K * M, 256)), dim3(256), 0, (hipStream_t)stream, y, x, auc, K, S, M);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
