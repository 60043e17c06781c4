// Per-word Grad-CAM of the captioning LM (include/cvcl_hip.h "Per-word Grad-CAM"): the device side of the multi-seed BPTT sweep.
// Every (caption, word) pair is one seed row whose gradient chain runs over the SAME saved gate activations of its caption; the seed
// state is laid out seed-major ([L][B][H]: block p holds the chains that started at position p), so the chains alive at step s are a
// contiguous tail and one launch + one recurrent GEMM serve all of them.  Both kernels are pure streaming passes in fp32.
#include "cvcl_common.h"

#include <math.h>

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// BPTT step s on `rows` seed rows (row r belongs to caption r % B and reads that caption's saved row b L + s).  Per element the
// arithmetic is lstm_cell_bwd_kernel's (csrc/vit.hip) / lstm_cell_bwd_first_kernel's (csrc/textgen.hip), four hidden units per lane.
// d_out != NULL: the first B rows are the chains that start at this step -- their dh is d_out[b L + s] (0 where the caption has
// ended) and their dc is 0, neither buffer is read for them.
__global__ __launch_bounds__(256) void lstm_cell_bwd_seeds_kernel(const float* __restrict__ gates_act, const float* __restrict__ c_save,
                                                                  const float* __restrict__ c0, const int64_t* __restrict__ len, int s,
                                                                  const float* __restrict__ d_out, float* __restrict__ dh,
                                                                  float* __restrict__ dc, float* __restrict__ d_gates,
                                                                  float* __restrict__ dh_carry, int B, int L, int Hd, long rows) {
    const int Hq = Hd >> 2;
    const long total = rows * Hq;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % Hq) << 2;
        const long r = i / Hq;
        const int b = (int)(r % B);
        const long srow = (long)b * L + s;
        const long off = r * Hd + j;
        const bool joins = d_out != nullptr && r < B;
        const bool live = len[b] > s;
        float* dg = d_gates + r * 4 * Hd + j;
        if (!live) {                                 // the step was not taken: h_s = h_{s-1}, c_s = c_{s-1}
            st4(dg, zero); st4(dg + Hd, zero); st4(dg + 2 * Hd, zero); st4(dg + 3 * Hd, zero);
            st4(dh_carry + off, joins ? zero : ld4(dh + off));
            if (joins) st4(dc + off, zero);
            continue;
        }
        const f32x4 dho = joins ? ld4(d_out + srow * Hd + j) : ld4(dh + off);
        const f32x4 dcv = joins ? zero : ld4(dc + off);
        const float* ga = gates_act + srow * 4 * Hd + j;
        const f32x4 ig = ld4(ga), fg = ld4(ga + Hd), gg = ld4(ga + 2 * Hd), og = ld4(ga + 3 * Hd);
        const f32x4 c_t = ld4(c_save + srow * Hd + j);
        const f32x4 c_prev = s > 0 ? ld4(c_save + (srow - 1) * Hd + j) : (c0 ? ld4(c0 + (long)b * Hd + j) : zero);
        f32x4 d_i, d_f, d_g, d_o, dcn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float tc = tanhf(c_t[e]);
            const float dct = dcv[e] + dho[e] * og[e] * (1.f - tc * tc);
            d_i[e] = dct * gg[e] * ig[e] * (1.f - ig[e]);
            d_f[e] = dct * c_prev[e] * fg[e] * (1.f - fg[e]);
            d_g[e] = dct * ig[e] * (1.f - gg[e] * gg[e]);
            d_o[e] = dho[e] * tc * og[e] * (1.f - og[e]);
            dcn[e] = dct * fg[e];
        }
        st4(dg, d_i); st4(dg + Hd, d_f); st4(dg + 2 * Hd, d_g); st4(dg + 3 * Hd, d_o);
        st4(dc + off, dcn);
        st4(dh_carry + off, zero);
    }
}

// Gradient rows of the sweep, seed-major (row p B + b), -> rows in image-major order (row b K + p) through the backward of
// F.normalize with the image's own (y, norm): l2norm_bwd_kernel's arithmetic (csrc/head.hip) with y / norm broadcast over the K
// seeds of an image.  y == NULL: the reordering alone.  One wave per row, 4 rows per workgroup.
__global__ __launch_bounds__(256) void l2norm_bwd_seeds_kernel(const float* __restrict__ y, const float* __restrict__ norm,
                                                               const float* __restrict__ dy, float* __restrict__ dx, int B, int K, int E,
                                                               float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * K) return;
    const int p = (int)(row / B), b = (int)(row % B);
    const float* gr = dy + row * E;
    float* out = dx + ((long)b * K + p) * E;
    if (y == nullptr) {
        for (int e = lane; e < E; e += 64) out[e] = gr[e];
        return;
    }
    const float* yr = y + (long)b * E;
    float dot = 0.f;
    for (int e = lane; e < E; e += 64) dot = fmaf(yr[e], gr[e], dot);
    dot = wave_sum(dot);
    const float nrm = norm[b];
    if (nrm < eps) {                 // clamp_min active: y = x / eps, no projection term
        for (int e = lane; e < E; e += 64) out[e] = gr[e] / eps;
    } else {
        for (int e = lane; e < E; e += 64) out[e] = (gr[e] - yr[e] * dot) / nrm;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int cvcl_lstm_cell_bwd_seeds(const float* gates_act, const float* c_save, const float* c0, const int64_t* len, int s,
                                        const float* d_out, float* dh, float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd,
                                        long rows, void* stream) {
    CVCL_CHECK_ARG(gates_act && c_save && len && dh && dc && d_gates && dh_carry, "cvcl_lstm_cell_bwd_seeds: null pointer");
    CVCL_CHECK_ARG(B >= 1 && L >= 1, "cvcl_lstm_cell_bwd_seeds: bad sizes (B %d, L %d)", B, L);
    CVCL_CHECK_ARG(Hd >= 4 && Hd % 4 == 0, "cvcl_lstm_cell_bwd_seeds: Hd %d is not a positive multiple of 4", Hd);
    CVCL_CHECK_ARG(s >= 0 && s < L, "cvcl_lstm_cell_bwd_seeds: step %d outside [0, %d)", s, L);
    CVCL_CHECK_ARG(rows >= 1 && rows % B == 0, "cvcl_lstm_cell_bwd_seeds: rows %ld is not a positive multiple of B %d", rows, B);
    CVCL_CHECK_ARG(rows / B <= L - s, "cvcl_lstm_cell_bwd_seeds: %ld seed blocks at step %d, at most %d can be alive", rows / B, s, L - s);
    CVCL_CHECK_ARG(!c0 || s == 0, "cvcl_lstm_cell_bwd_seeds: c0 belongs to step 0 (step %d)", s);
    CVCL_CHECK_ARG(aligned16(gates_act) && aligned16(c_save) && aligned16(c0) && aligned16(d_out) && aligned16(dh) && aligned16(dc) &&
                   aligned16(d_gates) && aligned16(dh_carry), "cvcl_lstm_cell_bwd_seeds: a buffer is not 16-byte aligned");
    CvclProfScope prof(stream, CVCL_K_LSTM);
    const long blocks = (rows * (Hd / 4) + 255) / 256;
    hipLaunchKernelGGL(lstm_cell_bwd_seeds_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                       gates_act, c_save, c0, len, s, d_out, dh, dc, d_gates, dh_carry, B, L, Hd, rows);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_l2norm_bwd_seeds(const float* y, const float* norm, const float* dy, float* dx, int B, int K, int E, float eps,
                                     void* stream) {
    CVCL_CHECK_ARG(dy && dx, "cvcl_l2norm_bwd_seeds: null pointer (dy / dx)");
    CVCL_CHECK_ARG((y == nullptr) == (norm == nullptr), "cvcl_l2norm_bwd_seeds: y and norm go together");
    CVCL_CHECK_ARG(dy != dx, "cvcl_l2norm_bwd_seeds: dx must not alias dy (the rows are reordered)");
    CVCL_CHECK_ARG(B >= 1 && K >= 1 && E >= 1, "cvcl_l2norm_bwd_seeds: bad sizes (B %d, K %d, E %d)", B, K, E);
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(l2norm_bwd_seeds_kernel, dim3(cvcl_div_up((long)B * K, 4)), dim3(256), 0, (hipStream_t)stream, y, norm, dy, dx, B,
                       K, E, eps);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
