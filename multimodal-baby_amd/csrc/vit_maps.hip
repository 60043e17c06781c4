// Self-attention maps of the DINO ViT (reference multimodal/vision_transformer_dino_mugs.py:252-259 get_last_selfattention, i.e. the
// softmax(q k^T * scale) of :123-124 WRITTEN OUT).  Every other attention kernel of the library keeps the probabilities in registers
// and writes only P V; this one writes P and nothing else.
//
//   cvcl_attention_probs     qkv [B][T][3][heads][hd] (fp32 or bf16) -> probs [B][heads][q_rows][T] fp32, queries 0 .. q_rows-1
//   cvcl_cls_attention_maps  the CLS query's row without its CLS column, per head or averaged over the heads
//   cvcl_attention_head_fuse the same softmax passes, folded over the heads (mean / max / min) -> F [B][T][T] fp32: the input of the
//                            attention rollout (csrc/vit_rollout.hip); no [B][heads][T][T] intermediate
//
// head_dim 64 (every DINO ViT), MFMA route.  One 256-thread workgroup owns (image, head, tile of 128 queries); each of its 4 waves owns
// 32 queries, whose q rows stay in registers as the MFMA A operand.  The keys stream through LDS in tiles of 64 (two buffers, one barrier
// per tile, the next tile's global loads in flight under this tile's MFMAs), so T is not limited by LDS.  S = Q K^T with the query in
// the accumulator ROW and the key in the lane's column (lane l: key l & 31; register r of lane half h: query (r & 3) + 8 (r >> 2) + 4 h),
// so that one store instruction writes two 128-byte runs along the key index of two rows.  fp32: v_mfma_f32_32x32x2_f32 (exact fp32,
// operand maps as csrc/vit_f32_train.hip); bf16: v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
//   pass 1: every lane keeps a running (max, sum) of the keys it sees for its 16 rows; the 32 lanes of a row are combined once, at
//           the end, in a fixed xor-shuffle order;
//   pass 2: the scores are rebuilt by the same instructions (bit-identical) and exp2((s - max) log2 e) / sum is stored -- exp2(s' -
//           lse) in the log2 units of cvcl_attention_train, with the subtraction done before the change of units and the division
//           kept apart from the exponent: both keep the error of a probability at that of its score (s - max is exact for the scores
//           that matter).
// No T x T scratch, no atomics, fixed reduction order: two runs are bit-identical.  The kernel is bound by its stores (4 T bytes per
// row: a row start is only 4-byte aligned at T = 197 / 257, so the stores are dwords, 32 consecutive per half wave).  They are PLAIN
// stores: the 128-byte runs straddle cache lines, and the L2 merges the partial lines of neighbouring runs before they leave for HBM
// (measured at B = 256, 12 heads, T = 197, bf16: 0.25 ms plain against 0.40 ms with nontemporal stores).
//
// Other head sizes (hd % 4 == 0, hd <= 128): a plain fp32 VALU route, one wave per query row, three passes (max, sum, store) that
// recompute the dot products in d order.  Correct, not fast: the goldens' 32-wide heads and unit tests use it.
#include "cvcl_common.h"

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_WAVES = AP_THREADS / 64;
constexpr int AP_QT = 32 * AP_WAVES;            // queries per workgroup
constexpr int AP_KT = 64;                       // keys per LDS tile
constexpr float AP_LOG2E = 1.4426950408889634f;

template <typename T> struct ApTraits;
template <> struct ApTraits<float> {
    static constexpr int kPitch = 68;           // LDS row pitch in elements (272 B: the 16-byte reads of 16 rows hit distinct banks)
    static constexpr int kSteps = 8;            // 16-byte operand reads per 32 x 32 score tile
    using Frag = f32x4;
};
template <> struct ApTraits<bf16_t> {
    static constexpr int kPitch = 72;           // 144 B (csrc/gemm.hip's pitch for 128-byte rows)
    static constexpr int kSteps = 4;
    using Frag = bf16x8;
};

__device__ __forceinline__ f32x16 ap_mma(f32x16 acc, const f32x4& a, const f32x4& b) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x16 ap_mma(f32x16 acc, const bf16x8& a, const bf16x8& b) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// One (image, head, tile of 128 queries): both softmax passes.  ``base`` is q of token 0 of that image and head (k at + D), q0 this
// wave's first query, sK the workgroup's two key buffers; emit(row, key, p) receives every probability of the rows < q_rows exactly
// once, row by row in runs of 32 keys per half wave.  Shared by cvcl_attention_probs (emit = a store) and cvcl_attention_head_fuse
// (emit = the fold into the head-fused tile).  A workgroup may call it again at once (the next head): the buffer a call stages first
// was last read before the previous call's final barrier, the other one before the barrier of the new call's first tile.
template <typename T, typename Emit>
__device__ __forceinline__ void ap_softmax_tile(T (&sK)[2][AP_KT * ApTraits<T>::kPitch], const T* __restrict__ base, int Tn, int D,
                                                float scale, int q_rows, int q0, Emit emit) {
    using Tr = ApTraits<T>;
    using Frag = typename Tr::Frag;
    constexpr int PER = ElemTraits<T>::kPerChunk;            // elements per 16-byte chunk
    constexpr int CPR = 64 / PER;                            // chunks per key row
    constexpr int NCH = AP_KT * CPR / AP_THREADS;            // chunks a thread stages per tile
    constexpr int RSTEP = AP_THREADS / CPR;                  // key rows between a thread's chunks

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const long rs = 3L * D;
    const int nkt = cvcl_div_up(Tn, AP_KT);
    const bool active = q0 < q_rows;                         // wave-uniform; idle waves still stage and meet the barriers

    // this wave's queries: lane (l31, h) holds the dims its half contracts, for query q0 + l31 (clamped: masked at the store)
    Frag qv[Tr::kSteps];
    {
        const int qrow = min(q0 + l31, q_rows - 1);
#pragma unroll
        for (int g = 0; g < Tr::kSteps; ++g) qv[g] = *reinterpret_cast<const Frag*>(base + (long)qrow * rs + (2 * g + h) * PER);
    }

    // staging role: chunk sc of key rows sr + i RSTEP of the tile
    const int sc = tid % CPR, sr = tid / CPR;
    Chunk<T> stg[NCH];
    auto fetch = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int key = min(kt * AP_KT + sr + i * RSTEP, Tn - 1);       // rows past T: a valid address, masked by key index
            stg[i].load(base + D + (long)key * rs + sc * PER);
        }
    };

    float m[16], l[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

    fetch(0);
    for (int st = 0; st < 2 * nkt; ++st) {
        const bool second = st >= nkt;
        const int kt = second ? st - nkt : st;
        T* buf = sK[st & 1];
#pragma unroll
        for (int i = 0; i < NCH; ++i) stg[i].store(buf + (sr + i * RSTEP) * Tr::kPitch + sc * PER);
        __syncthreads();       // one barrier per tile: the buffer written next was last read before THIS barrier by every wave
        if (st + 1 < 2 * nkt) fetch(st + 1 >= nkt ? st + 1 - nkt : st + 1);
        if (active) {
#pragma unroll
            for (int sub = 0; sub < AP_KT / 32; ++sub) {
                const int k0 = kt * AP_KT + sub * 32;
                if (k0 >= Tn) break;
                f32x16 s;
#pragma unroll
                for (int e = 0; e < 16; ++e) s[e] = 0.f;
                const T* kr = buf + (sub * 32 + l31) * Tr::kPitch + h * PER;
#pragma unroll
                for (int g = 0; g < Tr::kSteps; ++g) s = ap_mma(s, qv[g], *reinterpret_cast<const Frag*>(kr + 2 * g * PER));
                const int key = k0 + l31;
                if (key < Tn) {
                    if (!second) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {       // one exp2 per score: the smaller of (old max, score) is the one rescaled
                            const float t = s[r] * scale;
                            const float d = t - m[r];
                            const float e = __builtin_amdgcn_exp2f(-fabsf(d) * AP_LOG2E);
                            l[r] = d > 0.f ? fmaf(l[r], e, 1.f) : l[r] + e;
                            m[r] = fmaxf(m[r], t);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            const float p = __builtin_amdgcn_exp2f((s[r] * scale - m[r]) * AP_LOG2E) * l[r];
                            if (row < q_rows) emit(row, key, p);
                        }
                    }
                }
            }
        }
        if (st == nkt - 1) {
            // the 32 lanes of a row -> the row's max and 1 / sum (fixed order; lanes that saw no key carry (-inf, 0))
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float M = m[r];
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
                float v = l[r] * __builtin_amdgcn_exp2f((m[r] - M) * AP_LOG2E);
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
                m[r] = M;
                l[r] = 1.f / v;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(AP_THREADS) void attention_probs_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int Tn,
                                                                     int heads, float scale, int q_rows, int nqt) {
    __shared__ __attribute__((aligned(16))) T sK[2][AP_KT * ApTraits<T>::kPitch];
    const int wave = threadIdx.x >> 6;
    const int qt = blockIdx.x % nqt, hh = (blockIdx.x / nqt) % heads, b = blockIdx.x / (nqt * heads);
    const int D = heads * 64;
    float* out = probs + ((long)(b * heads + hh) * q_rows) * Tn;
    ap_softmax_tile<T>(sK, qkv + (long)b * Tn * 3L * D + hh * 64, Tn, D, scale, q_rows, qt * AP_QT + wave * 32,
                       [=](int row, int key, float p) { out[(long)row * Tn + key] = p; });
}

// cvcl_attention_head_fuse, MFMA route: one workgroup owns the [128 queries][T] tile of F[b] and visits the heads in index order.  A
// thread meets the same (row, key) in every head (the operand maps do not depend on the head), so it folds each head into ITS OWN
// elements of the tile in global memory: head 0 stores, the later heads read back what the same thread stored, no atomics, no
// barrier, no [heads][T][T] intermediate.  The tile (100 KB at T = 197) stays in the L2 between the heads.
enum { FUSE_MEAN = 0, FUSE_MAX = 1, FUSE_MIN = 2 };

__device__ __forceinline__ float fuse_fold(int fuse, float acc, float p) {
    return fuse == FUSE_MEAN ? acc + p : (fuse == FUSE_MAX ? fmaxf(acc, p) : fminf(acc, p));
}

template <typename T>
__global__ __launch_bounds__(AP_THREADS) void attention_head_fuse_kernel(const T* __restrict__ qkv, float* fused, int Tn, int heads,
                                                                         float scale, int fuse, float inv_heads, int nqt) {
    __shared__ __attribute__((aligned(16))) T sK[2][AP_KT * ApTraits<T>::kPitch];
    const int wave = threadIdx.x >> 6;
    const int qt = blockIdx.x % nqt, b = blockIdx.x / nqt;
    const int D = heads * 64;
    float* out = fused + (long)b * Tn * Tn;
    for (int hh = 0; hh < heads; ++hh) {
        const bool first = hh == 0, scale_now = fuse == FUSE_MEAN && hh == heads - 1;
        ap_softmax_tile<T>(sK, qkv + (long)b * Tn * 3L * D + hh * 64, Tn, D, scale, Tn, qt * AP_QT + wave * 32,
                           [=](int row, int key, float p) {
                               float* o = out + (long)row * Tn + key;
                               float v = first ? p : fuse_fold(fuse, *o, p);
                               if (scale_now) v *= inv_heads;
                               *o = v;
                           });
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// any head_dim % 4 == 0, <= 128: one wave per query row, the lanes stride over the keys; fp32 fmaf chains in d order
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int AV_MAXHD = 128;

// One query row on one wave: q [hd] fp32 (LDS), k of token 0 at ``kbase``; emit(key, p) receives the row's probabilities, lane l the
// keys l, l + 64, ...
template <typename T, typename Emit>
__device__ __forceinline__ void av_softmax_row(const float* q, const T* __restrict__ kbase, long rs, int hd, int Tn, float scale, Emit emit) {
    const int lane = threadIdx.x & 63;
    auto score = [&](int key) {
        const T* k = kbase + (long)key * rs;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(q[d], ElemTraits<T>::to_f(k[d]), s);
        return s * scale;
    };
    float M = -INFINITY;
    for (int key = lane; key < Tn; key += 64) M = fmaxf(M, score(key));
    M = wave_max(M);
    float L = 0.f;
    for (int key = lane; key < Tn; key += 64) L += __builtin_amdgcn_exp2f((score(key) - M) * AP_LOG2E);
    L = wave_sum(L);
    const float inv = 1.f / L;
    for (int key = lane; key < Tn; key += 64) emit(key, __builtin_amdgcn_exp2f((score(key) - M) * AP_LOG2E) * inv);
}

template <typename T>
__global__ __launch_bounds__(256) void attention_probs_valu_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int Tn, int heads,
                                                                   int hd, float scale, int q_rows, int nqt) {
    __shared__ float sQ[4][AV_MAXHD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x % nqt, hh = (blockIdx.x / nqt) % heads, b = blockIdx.x / (nqt * heads);
    const int D = heads * hd;
    const long rs = 3L * D;
    const T* base = qkv + (long)b * Tn * rs + hh * hd;
    const int row = qt * 4 + wave;
    const bool active = row < q_rows;
    if (active)
        for (int d = lane; d < hd; d += 64) sQ[wave][d] = ElemTraits<T>::to_f(base[(long)row * rs + d]);
    __syncthreads();
    if (!active) return;
    float* out = probs + ((long)(b * heads + hh) * q_rows + row) * Tn;
    av_softmax_row<T>(sQ[wave], base + D, rs, hd, Tn, scale, [=](int key, float p) { out[key] = p; });
}

// cvcl_attention_head_fuse, VALU route: one wave per row of F[b], the heads in index order; a lane folds into its own keys.
template <typename T>
__global__ __launch_bounds__(256) void attention_head_fuse_valu_kernel(const T* __restrict__ qkv, float* fused, int Tn, int heads, int hd,
                                                                       float scale, int fuse, float inv_heads, int nqt) {
    __shared__ float sQ[4][AV_MAXHD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x % nqt, b = blockIdx.x / nqt;
    const int D = heads * hd;
    const long rs = 3L * D;
    const int row = qt * 4 + wave;
    const bool active = row < Tn;
    float* out = fused + ((long)b * Tn + row) * Tn;
    for (int hh = 0; hh < heads; ++hh) {
        const T* base = qkv + (long)b * Tn * rs + hh * hd;
        __syncthreads();                                     // the previous head's reads of sQ
        if (active)
            for (int d = lane; d < hd; d += 64) sQ[wave][d] = ElemTraits<T>::to_f(base[(long)row * rs + d]);
        __syncthreads();
        if (!active) continue;
        const bool first = hh == 0, scale_now = fuse == FUSE_MEAN && hh == heads - 1;
        av_softmax_row<T>(sQ[wave], base + D, rs, hd, Tn, scale, [=](int key, float p) {
            float v = first ? p : fuse_fold(fuse, out[key], p);
            if (scale_now) v *= inv_heads;
            out[key] = v;
        });
    }
}

// probs [B][heads][1][T] -> out [B][T-1] (mean over the heads, h = 0 first) or out [B][heads][T-1] (a copy without column 0)
__global__ __launch_bounds__(256) void cls_maps_kernel(const float* __restrict__ probs, float* __restrict__ out, int heads, int Tn,
                                                       int mean, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int np = Tn - 1;
    if (mean) {
        const long b = i / np;
        const int j = (int)(i - b * np);
        const float* src = probs + b * heads * Tn + 1 + j;
        float s = 0.f;
        for (int hh = 0; hh < heads; ++hh) s += src[(long)hh * Tn];
        out[i] = s / (float)heads;
    } else {
        const long bh = i / np;
        out[i] = probs[bh * Tn + 1 + (i - bh * np)];
    }
}

}  // namespace

extern "C" int cvcl_attention_probs(int dtype, const void* qkv, float* probs, int B, int T, int heads, int head_dim, float scale,
                                    int q_rows, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_attention_probs");
    CVCL_CHECK_ARG(qkv && probs, "cvcl_attention_probs: null qkv / probs");
    CVCL_CHECK_ARG(B > 0 && T > 0 && heads > 0, "cvcl_attention_probs: sizes must be positive (B %d T %d heads %d)", B, T, heads);
    CVCL_CHECK_ARG(q_rows >= 1 && q_rows <= T, "cvcl_attention_probs: q_rows %d outside 1 .. T = %d", q_rows, T);
    CVCL_CHECK_ARG(head_dim > 0 && head_dim % 4 == 0 && head_dim <= AV_MAXHD,
                   "cvcl_attention_probs: head_dim %d is not a multiple of 4 in 4 .. %d", head_dim, AV_MAXHD);
    CVCL_CHECK_ARG(scale == scale && scale - scale == 0.f, "cvcl_attention_probs: scale must be finite");
    const bool mfma = head_dim == 64;
    const int nqt = cvcl_div_up(q_rows, mfma ? AP_QT : 4);
    const long grid = (long)B * heads * nqt;
    CVCL_CHECK_ARG(grid <= 0x7fffffffL, "cvcl_attention_probs: grid of %ld workgroups is too large", grid);
    CVCL_CHECK_ARG(!mfma || cvcl_aligned16(qkv), "cvcl_attention_probs: qkv must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    if (mfma) {
        if (dtype == CVCL_F32)
            hipLaunchKernelGGL(attention_probs_kernel<float>, dim3((unsigned)grid), dim3(AP_THREADS), 0, s, (const float*)qkv, probs, T, heads,
                               scale, q_rows, nqt);
        else
            hipLaunchKernelGGL(attention_probs_kernel<bf16_t>, dim3((unsigned)grid), dim3(AP_THREADS), 0, s, (const bf16_t*)qkv, probs, T,
                               heads, scale, q_rows, nqt);
    } else {
        if (dtype == CVCL_F32)
            hipLaunchKernelGGL(attention_probs_valu_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, (const float*)qkv, probs, T, heads,
                               head_dim, scale, q_rows, nqt);
        else
            hipLaunchKernelGGL(attention_probs_valu_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)qkv, probs, T, heads,
                               head_dim, scale, q_rows, nqt);
    }
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_attention_head_fuse(int dtype, const void* qkv, float* fused, int B, int T, int heads, int head_dim, float scale,
                                        int fuse, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_attention_head_fuse");
    CVCL_CHECK_ARG(qkv && fused, "cvcl_attention_head_fuse: null qkv / fused");
    CVCL_CHECK_ARG(B > 0 && T > 0 && heads > 0, "cvcl_attention_head_fuse: sizes must be positive (B %d T %d heads %d)", B, T, heads);
    CVCL_CHECK_ARG(head_dim > 0 && head_dim % 4 == 0 && head_dim <= AV_MAXHD,
                   "cvcl_attention_head_fuse: head_dim %d is not a multiple of 4 in 4 .. %d", head_dim, AV_MAXHD);
    CVCL_CHECK_ARG(scale == scale && scale - scale == 0.f, "cvcl_attention_head_fuse: scale must be finite");
    CVCL_CHECK_ARG(fuse == CVCL_FUSE_MEAN || fuse == CVCL_FUSE_MAX || fuse == CVCL_FUSE_MIN,
                   "cvcl_attention_head_fuse: fuse %d is not CVCL_FUSE_MEAN / MAX / MIN", fuse);
    static_assert(CVCL_FUSE_MEAN == FUSE_MEAN && CVCL_FUSE_MAX == FUSE_MAX && CVCL_FUSE_MIN == FUSE_MIN, "fuse codes");
    const bool mfma = head_dim == 64;
    const int nqt = cvcl_div_up(T, mfma ? AP_QT : 4);
    const long grid = (long)B * nqt;
    CVCL_CHECK_ARG(grid <= 0x7fffffffL, "cvcl_attention_head_fuse: grid of %ld workgroups is too large", grid);
    CVCL_CHECK_ARG(!mfma || cvcl_aligned16(qkv), "cvcl_attention_head_fuse: qkv must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const float inv_heads = 1.f / (float)heads;
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    if (mfma) {
        if (dtype == CVCL_F32)
            hipLaunchKernelGGL(attention_head_fuse_kernel<float>, dim3((unsigned)grid), dim3(AP_THREADS), 0, s, (const float*)qkv, fused, T,
                               heads, scale, fuse, inv_heads, nqt);
        else
            hipLaunchKernelGGL(attention_head_fuse_kernel<bf16_t>, dim3((unsigned)grid), dim3(AP_THREADS), 0, s, (const bf16_t*)qkv, fused,
                               T, heads, scale, fuse, inv_heads, nqt);
    } else {
        if (dtype == CVCL_F32)
            hipLaunchKernelGGL(attention_head_fuse_valu_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, (const float*)qkv, fused, T,
                               heads, head_dim, scale, fuse, inv_heads, nqt);
        else
            hipLaunchKernelGGL(attention_head_fuse_valu_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)qkv, fused, T,
                               heads, head_dim, scale, fuse, inv_heads, nqt);
    }
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_cls_attention_maps(const float* probs, float* out, int B, int heads, int T, int mean, void* stream) {
    CVCL_CHECK_ARG(probs && out, "cvcl_cls_attention_maps: null probs / out");
    CVCL_CHECK_ARG(probs != out, "cvcl_cls_attention_maps: out must not alias probs");
    CVCL_CHECK_ARG(B > 0 && heads > 0 && T > 1, "cvcl_cls_attention_maps: needs B, heads > 0 and T > 1 (B %d heads %d T %d)", B, heads, T);
    const long total = (long)B * (mean ? 1 : heads) * (T - 1);
    CVCL_CHECK_ARG((total + 255) / 256 <= 0x7fffffffL, "cvcl_cls_attention_maps: grid too large");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(cls_maps_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, probs, out, heads, T,
                       mean ? 1 : 0, total);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
