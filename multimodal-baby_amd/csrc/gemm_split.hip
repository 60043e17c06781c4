// Split-bf16 GEMM for fp32 operands: the 1x1 convolutions and downsample products of the CVCL_F32X3 ("32-split") trunk.
//
//      C[M,N] = A[M,K] . W[N,K]^T        A, C fp32 row-major; W packed by cvcl_pack_conv_weight(CVCL_F32X3, CVCL_PACK_DENSE)
//
// Arithmetic: every fp32 operand x is written as a sum of bf16 parts, x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), and
// the product a.w is formed from the part products of rank i + j <= NT / 3 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
// (a product of two bf16 numbers is exact in fp32):
//   NT = 3:  a0 w0 + a1 w0 + a0 w1                      (drops a1 w1 <= 2^-18 and the split remainder <= 2^-17: ~2^-16 relative)
//   NT = 6:  ... + a0 w2 + a1 w1 + a2 w0                (three-way split of both operands: ~fp32)
// W is split once, when it is packed ([P][N][ldw] bf16, P = 2 or 3 parts); A is split as it is staged into LDS.
//
// Structure (CDNA4): 128 x 128 output tile per 256-thread workgroup (4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles), K tile 32;
// the next K tile's global loads are in flight in registers while the current one is multiplied out of LDS.  MFMA-A = activation
// rows, MFMA-B = weight rows, so a lane owns ONE output channel of 16 rows per tile: the per-channel BatchNorm partial sums of the
// stored values are kept in two registers per n-tile across all M tiles of the (persistent) workgroup and written once as a
// partial row -- deterministic, no atomics, and no separate statistics pass over the output.
#include "cvcl_common.h"

namespace {

constexpr int SP_BM = 128, SP_BN = 128, SP_BK = 32;
constexpr int SP_PITCH = 80;                      // LDS row pitch: 64 B of K + 16 B pad (the 16 rows of a ds_read_b128 hit 16 slots)
constexpr int SP_TILE = SP_BM * SP_PITCH;         // one part of one operand tile

template <int NT> struct SplitTerms {
    static_assert(NT == 3 || NT == 6, "3 or 6 split terms");
    static constexpr int P = NT == 3 ? 2 : 3;     // bf16 parts per operand
};

template <int NT> constexpr int split_lds_bytes() { return 2 * SplitTerms<NT>::P * SP_TILE + 2 * 2 * SP_BN * 4; }

struct SplitDev {
    const float* A; const bf16_t* W; float* C; float* stats;
    int M, N, K, lda, ldw, ldc;
    long w_part;                          // elements between two weight parts (N * ldw)
    int gs, g_hw, g_wo, g_hi, g_wi;       // row gather of a strided 1x1 convolution (gs <= 1: off)
    int tiles_m;
};

// bf16 parts of x (see the top).  A finite x beyond the bf16 range keeps the largest finite bf16 as its first part (the rest is then
// representable); a non-finite x is its own first part with zero remainders.  Selects only (loads are in flight around the call).
template <int P>
__device__ __forceinline__ void split_parts(float x, bf16_t* part) {
    const bf16_t h0 = (bf16_t)x;
    const bool hfin = __builtin_isfinite((float)h0), xfin = __builtin_isfinite(x);
    const bf16_t hmax = __builtin_bit_cast(bf16_t, (unsigned short)(x < 0.f ? 0xFF7F : 0x7F7F));
    const bf16_t h = (!hfin && xfin) ? hmax : h0;
    part[0] = h;
    float r = xfin ? x - (float)h : 0.f;
#pragma unroll
    for (int i = 1; i < P; ++i) {
        part[i] = (bf16_t)r;
        r -= (float)part[i];
    }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void gemm_split_kernel(SplitDev p) {
    constexpr int P = SplitTerms<NT>::P;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                                      // [P][128 rows][SP_PITCH]
    char* sW = smem + P * SP_TILE;                        // [P][128 rows][SP_PITCH]
    float* red = reinterpret_cast<float*>(smem + 2 * P * SP_TILE);     // [2 wm][2 (sum, sumsq)][128 columns]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int r32 = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.y * SP_BN;
    const int ktiles = p.K / SP_BK;

    // staging: A chunk c = tid + 256 i (i < 4) is row c >> 3, columns (c & 7) * 4 .. +3; W chunk c = tid + 256 j (j < 2) of every part is
    // row c >> 2, columns (c & 3) * 8 .. +7
    long a_off[4];
    f32x4 ra[4];
    u32x4 rw[P][2];
    const bf16_t* wsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = tid + 256 * j;
        wsrc[j] = p.W + (long)(n0 + (c >> 2)) * p.ldw + (c & 3) * 8;
    }
    float s_acc[2] = {0.f, 0.f}, q_acc[2] = {0.f, 0.f};

    auto gload = [&](int kt) {
        const int k0 = kt * SP_BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const f32x4*>(p.A + a_off[i] + k0);
#pragma unroll
        for (int pt = 0; pt < P; ++pt)
#pragma unroll
            for (int j = 0; j < 2; ++j) rw[pt][j] = *reinterpret_cast<const u32x4*>(wsrc[j] + pt * p.w_part + k0);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            bf16_t prt[4][P];
#pragma unroll
            for (int e = 0; e < 4; ++e) split_parts<P>(ra[i][e], prt[e]);
#pragma unroll
            for (int pt = 0; pt < P; ++pt) {
                const bf16x4 v = {prt[0][pt], prt[1][pt], prt[2][pt], prt[3][pt]};
                *reinterpret_cast<bf16x4*>(sA + pt * SP_TILE + (c >> 3) * SP_PITCH + (c & 7) * 8) = v;
            }
        }
#pragma unroll
        for (int pt = 0; pt < P; ++pt)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = tid + 256 * j;
                *reinterpret_cast<u32x4*>(sW + pt * SP_TILE + (c >> 2) * SP_PITCH + (c & 3) * 16) = rw[pt][j];
            }
    };

    for (int tm = blockIdx.x; tm < p.tiles_m; tm += gridDim.x) {
        const int m0 = tm * SP_BM;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            const int m = min(m0 + (c >> 3), p.M - 1);    // rows past M re-read row M - 1 (masked at the store)
            long row = m;
            if (p.gs > 1) {
                const int b = m / p.g_hw, rem = m - b * p.g_hw, oy = rem / p.g_wo, ox = rem - oy * p.g_wo;
                row = ((long)b * p.g_hi + (long)oy * p.gs) * p.g_wi + (long)ox * p.gs;
            }
            a_off[i] = row * p.lda + (c & 7) * 4;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

        gload(0);
        for (int kt = 0; kt < ktiles; ++kt) {
            __syncthreads();                              // every wave is done with the previous tile's fragments
            lstore();
            __syncthreads();
            if (kt + 1 < ktiles) gload(kt + 1);           // in flight during the MFMAs below
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[2][P], fw[2][P];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int pt = 0; pt < P; ++pt)
                        fa[mi][pt] = *reinterpret_cast<const bf16x8*>(sA + pt * SP_TILE + (wm * 64 + mi * 32 + r32) * SP_PITCH + ks * 32 + h * 16);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int pt = 0; pt < P; ++pt)
                        fw[ni][pt] = *reinterpret_cast<const bf16x8*>(sW + pt * SP_TILE + (wn * 64 + ni * 32 + r32) * SP_PITCH + ks * 32 + h * 16);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        f32x16 c = acc[mi][ni];
                        // smallest terms first: they are added to the smaller partial sum
                        if constexpr (NT == 6) {
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][2], fw[ni][0], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][1], fw[ni][1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fw[ni][2], c, 0, 0, 0);
                        }
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][1], fw[ni][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fw[ni][1], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fw[ni][0], c, 0, 0, 0);
                        acc[mi][ni] = c;
                    }
            }
        }
        // epilogue: lane (r32, h) holds column n = n0 + wn 64 + ni 32 + r32 of rows (reg & 3) + 8 (reg >> 2) + 4 h of each 32-row tile;
        // for a fixed register the 32 lanes of a half write 128 contiguous bytes of one row
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int n = n0 + wn * 64 + ni * 32 + r32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < p.M) {
                        const float v = acc[mi][ni][r];
                        if (p.C) p.C[(long)m * p.ldc + n] = v;
                        s_acc[ni] += v;
                        q_acc[ni] = fmaf(v, v, q_acc[ni]);
                    }
                }
            }
    }
    if (!p.stats) return;
    // partial row blockIdx.x: lane halves h = 0 / 1, then the two waves of a column block (wm = 0 / 1), in a fixed order
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        s_acc[ni] += __shfl_xor(s_acc[ni], 32, 64);
        q_acc[ni] += __shfl_xor(q_acc[ni], 32, 64);
        if (h == 0) {
            const int col = wn * 64 + ni * 32 + r32;
            red[(wm * 2 + 0) * SP_BN + col] = s_acc[ni];
            red[(wm * 2 + 1) * SP_BN + col] = q_acc[ni];
        }
    }
    __syncthreads();
    if (tid < SP_BN) {
        const float s = red[0 * SP_BN + tid] + red[2 * SP_BN + tid];
        const float q = red[1 * SP_BN + tid] + red[3 * SP_BN + tid];
        cvcl_bn_stats_out(p.stats, 0, blockIdx.x, p.N, n0 + tid, s, q);
    }
}

template <int P>
__global__ void pack_split_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        bf16_t prt[P];
        split_parts<P>(w[i], prt);
#pragma unroll
        for (int pt = 0; pt < P; ++pt) out[pt * n + i] = prt[pt];
    }
}

// NT = 3 instantiated as well, so that the 3-term form keeps compiling
template __global__ void gemm_split_kernel<3>(SplitDev);

int split_grid_m(int M, int N) {
    static int cus = 0;
    if (!cus) {
        int dev = 0, c = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus = c;
    }
    const int tiles_m = cvcl_div_up(M, SP_BM), tiles_n = N / SP_BN;
    int g = cvcl_div_up(2L * cus, tiles_n);               // two workgroups per CU in total
    if (g > tiles_m) g = tiles_m;
    if (g > 1024) g = 1024;
    return g < 1 ? 1 : g;
}

template <int NT>
int launch_split(const SplitDev& d, int gm, hipStream_t stream) {
    static CvclLdsAttr attr;
    if (const int rc = cvcl_raise_lds_limit(attr, (const void*)gemm_split_kernel<NT>, split_lds_bytes<NT>(), "cvcl_gemm")) return rc;
    attr.mark();
    hipLaunchKernelGGL(gemm_split_kernel<NT>, dim3(gm, d.N / SP_BN), dim3(256), split_lds_bytes<NT>(), stream, d);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

}  // namespace

// number of BN partial rows cvcl_gemm(CVCL_F32X3) writes
int cvcl_gemm_split_stats_rows(int M, int N) { return M > 0 && N >= SP_BN ? split_grid_m(M, N) : 0; }

size_t cvcl_split_dense_bytes(long elems) { return (size_t)elems * kSplitParts * 2; }

int cvcl_pack_split_dense(const float* w, void* out, long elems, void* stream) {
    CVCL_CHECK_ARG(w && out && elems > 0, "cvcl_pack_conv_weight: bad args");
    const long g = cvcl_div_up(elems, 256);
    hipLaunchKernelGGL(pack_split_kernel<kSplitParts>, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, (hipStream_t)stream, w,
                       (bf16_t*)out, elems);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_gemm_split(const cvcl_gemm_args* a, void* stream) {
    CVCL_CHECK_ARG(!a->a_scale && !a->bias && !a->exp_scale && !a->R && !a->c_scale && !a->centre && !a->C_pre && !a->G && !a->A2 &&
                       !a->a_trans && !a->w_trans && !a->a_rowsum && !a->f32_split && !a->ln_stats && !a->ln_colsum && !a->row_part &&
                       a->act == CVCL_ACT_NONE,
                   "cvcl_gemm(CVCL_F32X3): plain products (+ BN statistics, row gather) only");
    CVCL_CHECK_ARG(a->N % SP_BN == 0 && a->K % SP_BK == 0 && a->lda % 4 == 0 && a->ldw % 8 == 0 && a->ldw >= a->K && a->lda >= a->K &&
                       (!a->C || a->ldc >= a->N) && cvcl_aligned16(a->A) && cvcl_aligned16(a->W),
                   "cvcl_gemm(CVCL_F32X3): needs N %% 128 == 0, K %% 32 == 0, lda %% 4 == 0, ldw %% 8 == 0 and 16-byte aligned A / W "
                   "(M %d N %d K %d lda %d ldw %d)", a->M, a->N, a->K, a->lda, a->ldw);
    const int gm = split_grid_m(a->M, a->N);
    CVCL_CHECK_ARG(!a->stats || (a->stats_rows != CVCL_STATS_ACCUMULATE && a->stats_rows >= gm),
                   "cvcl_gemm(CVCL_F32X3): stats_rows %d < %d (partial rows only)", a->stats_rows, gm);
    SplitDev d = {};
    d.A = (const float*)a->A; d.W = (const bf16_t*)a->W; d.C = (float*)a->C; d.stats = a->stats;
    d.M = a->M; d.N = a->N; d.K = a->K; d.lda = a->lda; d.ldw = a->ldw; d.ldc = a->ldc;
    d.w_part = (long)a->N * a->ldw;
    d.gs = 0;
    if (a->gather_stride > 1) {
        CVCL_CHECK_ARG(a->gather_ho > 0 && a->gather_wo > 0 && a->gather_hi > 0 && a->gather_wi > 0 &&
                           a->M % (a->gather_ho * a->gather_wo) == 0 && (a->gather_ho - 1) * a->gather_stride < a->gather_hi &&
                           (a->gather_wo - 1) * a->gather_stride < a->gather_wi,
                       "cvcl_gemm(CVCL_F32X3): bad row gather");
        d.gs = a->gather_stride; d.g_hw = a->gather_ho * a->gather_wo; d.g_wo = a->gather_wo; d.g_hi = a->gather_hi; d.g_wi = a->gather_wi;
    }
    d.tiles_m = cvcl_div_up(a->M, SP_BM);
    CvclProfScope prof(stream, CVCL_K_GEMM_F32);
    return launch_split<kSplitTerms>(d, gm, (hipStream_t)stream);
}
