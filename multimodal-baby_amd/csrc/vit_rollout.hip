// Attention rollout of the DINO ViT (Abnar & Zuidema 2020): the chain over the head-fused attention of the blocks.
//
//   cvcl_attention_rollout   F [n_layers][B][T][T] fp32 (cvcl_attention_head_fuse, csrc/vit_maps.hip, layer 0 = the earliest block)
//                            -> R [B][q_rows][T] fp32, the first q_rows rows of  A^_{n-1} . A^_{n-2} ... A^_{start_layer},
//                            A^_l = (F_l + I) / rowsum(F_l + I)
//
// One 256-thread workgroup owns (image, tile of RT rows of R); the rows live in LDS as two buffers [RT][T] that swap roles per layer,
// next to the T row sums of the layer at hand.  Per layer:
//   1. row sums: one wave per row of F_l, the lanes stride over j (coalesced), lane partials and the fixed xor-shuffle tree in fp64,
//      + 1 for the diagonal, rounded to fp32 once.  Computed, never assumed to be 2 (max / min fusion);
//   2. w[q][i] = r[q][i] / rowsum[i] in place: A^ is never stored, the normalisation rides on the row vector;
//   3. r'[q][j] = sum_i w[q][i] F_l[i][j] + w[q][j]: thread j walks i = 0 .. T-1 in order, its loads of F_l[i][.] coalesced along j,
//      w[q][i] an LDS broadcast, the RT accumulators in fp64 (the product of two fp32 is exact there, so a row of R carries one
//      rounding per layer instead of T), the diagonal term last.
// The rows start as rows q0 .. q0 + RT - 1 of A^_{n-1}.  Every row is computed by the same instruction sequence whatever its tile, so
// q_rows = 1 (RT = 1: one accumulator, 3 T floats of LDS) gives the bits of row 0 of q_rows = T (RT = 8).  No atomics, no workspace.
// LDS: (2 RT + 1) T floats <= 64 KB  ->  T <= 960 (T = 785, ViT-B/8 at 224 x 224: 53 KB, one workgroup per CU for the tiled form).
#include "cvcl_common.h"

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_RT = 8;                        // rows per workgroup when q_rows > 1
constexpr int RO_MAXT = 960;                    // (2 RO_RT + 1) T floats of LDS <= 64 KB

// rs[k] = 1 + sum_j Fl[(row0 + k) T + j] for k < n: wave w takes rows w, w + 4, ...
__device__ __forceinline__ void ro_row_sums(const float* __restrict__ Fl, int Tn, int row0, int n, float* rs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < n; k += RO_WAVES) {
        const float* row = Fl + (long)(row0 + k) * Tn;
        double s = 0.0;
        for (int j = lane; j < Tn; j += 64) s += (double)row[j];
        s = wave_sum(s);
        if (lane == 0) rs[k] = (float)(s + 1.0);
    }
}

template <int RT>
__global__ __launch_bounds__(RO_THREADS) void attention_rollout_kernel(const float* __restrict__ F, float* __restrict__ out, int n_layers,
                                                                       long layer_stride, int Tn, int start_layer, int q_rows, int nrt) {
    extern __shared__ float ro_smem[];
    float* rs = ro_smem;                         // [Tn]
    float* cur = ro_smem + Tn;                   // [RT][Tn]
    float* nxt = cur + RT * Tn;                  // [RT][Tn]
    const int tid = threadIdx.x;
    const int rt = blockIdx.x % nrt, b = blockIdx.x / nrt;
    const int q0 = rt * RT, nq = min(RT, q_rows - q0);
    const float* Fb = F + (long)b * Tn * Tn;

    // rows q0 .. q0 + nq - 1 of the last layer's A^; the rows past q_rows are zeros and stay zeros
    const float* Fl = Fb + (long)(n_layers - 1) * layer_stride;
    ro_row_sums(Fl, Tn, q0, nq, rs);
    __syncthreads();
    for (int idx = tid; idx < RT * Tn; idx += RO_THREADS) {
        const int q = idx / Tn, j = idx - q * Tn, row = q0 + q;
        cur[idx] = q < nq ? (Fl[(long)row * Tn + j] + (j == row ? 1.f : 0.f)) / rs[q] : 0.f;
    }
    __syncthreads();

    for (int l = n_layers - 2; l >= start_layer; --l) {
        Fl = Fb + (long)l * layer_stride;
        ro_row_sums(Fl, Tn, 0, Tn, rs);
        __syncthreads();
        for (int idx = tid; idx < RT * Tn; idx += RO_THREADS) cur[idx] = cur[idx] / rs[idx % Tn];
        __syncthreads();
        for (int j = tid; j < Tn; j += RO_THREADS) {
            double acc[RT];
#pragma unroll
            for (int q = 0; q < RT; ++q) acc[q] = 0.0;
            const float* col = Fl + j;
#pragma unroll 8
            for (int i = 0; i < Tn; ++i) {
                const double f = (double)col[(long)i * Tn];
#pragma unroll
                for (int q = 0; q < RT; ++q) acc[q] += (double)cur[q * Tn + i] * f;
            }
#pragma unroll
            for (int q = 0; q < RT; ++q) nxt[q * Tn + j] = (float)(acc[q] + (double)cur[q * Tn + j]);
        }
        __syncthreads();                         // nxt complete, cur and rs free
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    float* o = out + ((long)b * q_rows + q0) * Tn;
    for (int idx = tid; idx < nq * Tn; idx += RO_THREADS) o[idx] = cur[idx];
}

}  // namespace

extern "C" int cvcl_attention_rollout(const float* fused, float* out, int n_layers, int B, int T, int start_layer, int q_rows,
                                      void* stream) {
    CVCL_CHECK_ARG(fused && out, "cvcl_attention_rollout: null fused / out");
    CVCL_CHECK_ARG(fused != out, "cvcl_attention_rollout: out must not alias fused");
    CVCL_CHECK_ARG(n_layers >= 1, "cvcl_attention_rollout: n_layers %d < 1", n_layers);
    CVCL_CHECK_ARG(B > 0 && T > 0, "cvcl_attention_rollout: sizes must be positive (B %d T %d)", B, T);
    CVCL_CHECK_ARG(T <= RO_MAXT, "cvcl_attention_rollout: T %d > %d (the row tile's LDS)", T, RO_MAXT);
    CVCL_CHECK_ARG(start_layer >= 0 && start_layer < n_layers, "cvcl_attention_rollout: start_layer %d outside 0 .. n_layers - 1 = %d",
                   start_layer, n_layers - 1);
    CVCL_CHECK_ARG(q_rows >= 1 && q_rows <= T, "cvcl_attention_rollout: q_rows %d outside 1 .. T = %d", q_rows, T);
    const int rt = q_rows == 1 ? 1 : RO_RT;
    const int nrt = cvcl_div_up(q_rows, rt);
    const long grid = (long)B * nrt;
    CVCL_CHECK_ARG(grid <= 0x7fffffffL, "cvcl_attention_rollout: grid of %ld workgroups is too large", grid);
    const long layer_stride = (long)B * T * T;
    const size_t lds = (size_t)(2 * rt + 1) * T * sizeof(float);
    const hipStream_t s = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    if (rt == 1)
        hipLaunchKernelGGL(attention_rollout_kernel<1>, dim3((unsigned)grid), dim3(RO_THREADS), lds, s, fused, out, n_layers, layer_stride,
                           T, start_layer, q_rows, nrt);
    else
        hipLaunchKernelGGL(attention_rollout_kernel<RO_RT>, dim3((unsigned)grid), dim3(RO_THREADS), lds, s, fused, out, n_layers,
                           layer_stride, T, start_layer, q_rows, nrt);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
