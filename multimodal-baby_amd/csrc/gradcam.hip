// Grad-CAM for the flat ResNeXt encoder (reference multimodal/attention_maps.py:112-165).
//
// For layer = layer4, out = fc(avgpool(A)) (optionally L2-normalised) and out.backward(t), the gradient at the map is the same at
// every position, so the map of image n for target t_m is one contraction over the channels of the NHWC map rows:
//   cam[n, m, p] = relu((R[n, m, p] - s[n, m] U[n, p]) / (||f_n|| hw))     (normalised features; relu(R / hw) otherwise)
//   R[n, m, p] = sum_c P[m, c] A[n, p, c],  P = T W;   U[n, p] = sum_c Q[n, c] A[n, p, c],  Q = n^_n W;   s = n^ . t
// (derivation: DESIGN.md section 5, "Grad-CAM").  R and s U cancel where the target is close to the feature, so the contraction runs
// on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) in both storage modes: a bf16 map is widened exactly while it is staged.
//
// Kernels: the pair contraction + epilogue (all pairs, or the pairs of a block layout), torch's bicubic resize (align_corners=False),
// the generic gradCAM_with_act_and_grad over any layer's act / grad.  The avgpool backward of the hook bridge is cvcl_avgpool_bwd.
#include "cvcl_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// pair contraction: 64 map rows x 64 targets per 256-thread workgroup, K (channels) in steps of 32 staged through LDS as fp32;
// each wave owns a 32 x 32 quarter (one 32x32x2 f32 MFMA accumulator).  U of the tile's rows is accumulated by the staging threads
// from the same map registers (no second read of the map).  Grid: x = target tiles (fastest, so the workgroups of one row tile run
// together and the map is read from HBM about once), y = row tiles.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int GC_TILE = 64;
constexpr int GC_K = 32;
constexpr int GC_LD = GC_K + 1;                      // padded LDS row (floats): the 32 rows a half-wave reads fall in distinct banks

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}

template <typename T>
__global__ __launch_bounds__(256) void gradcam_pairs_kernel(const T* __restrict__ map, int N, int HW, int C,
                                                            const float* __restrict__ P, int M, int mode, int k,
                                                            const float* __restrict__ Q, const float* __restrict__ S,
                                                            const float* __restrict__ norm, float eps, float* __restrict__ cam,
                                                            int row_tiles_per_image) {
    __shared__ float sA[GC_TILE * GC_LD];
    __shared__ float sP[GC_TILE * GC_LD];
    __shared__ float sU[GC_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, h = lane >> 5;
    const bool all = mode == CVCL_GRADCAM_ALL;
    // row tile -> image (block layouts: one image per tile) and first position
    int n_tile = 0, p0 = 0;
    long r0 = 0;
    if (all) {
        r0 = (long)blockIdx.y * GC_TILE;
    } else {
        n_tile = blockIdx.y / row_tiles_per_image;
        p0 = (blockIdx.y % row_tiles_per_image) * GC_TILE;
        r0 = (long)n_tile * HW + p0;
    }
    const long rows_end = all ? (long)N * HW : (long)n_tile * HW + HW;
    const int cnt = all ? M : (mode == CVCL_GRADCAM_BLOCK_IMAGE ? k : 1);      // targets per image
    const int c0 = blockIdx.x * GC_TILE;
    auto target_of = [&](int n, int c) -> int {
        return all ? c : (mode == CVCL_GRADCAM_BLOCK_IMAGE ? n * k + c : n / k);
    };

    // staging role: row / target i of the tile, channels kc .. kc + 7 of the K step
    const int si = tid >> 2, kc = (tid & 3) * 8;
    const long sr = r0 + si;
    const bool srow_ok = sr < rows_end;
    const int sn = srow_ok ? (int)(sr / HW) : 0;
    const bool stgt_ok = c0 + si < cnt;
    const T* a_src = map + (srow_ok ? sr : 0) * (long)C + kc;
    const float* p_src = P + (long)(stgt_ok ? target_of(all ? 0 : n_tile, c0 + si) : 0) * C + kc;
    const float* q_src = Q ? Q + (long)sn * C + kc : nullptr;

    float ra[8], rp[8], u = 0.f;
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        if (srow_ok) load8(a_src + k0, ra);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ra[e] = 0.f;
        }
        if (stgt_ok) load8(p_src + k0, rp);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) rp[e] = 0.f;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < C; k0 += GC_K) {
        __syncthreads();                              // the previous step's operand reads are done
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sA[si * GC_LD + kc + e] = ra[e];
            sP[si * GC_LD + kc + e] = rp[e];
        }
        if (q_src && srow_ok) {                       // U from the staged map values (fp32 dot, fixed order)
            float q[8];
            load8(q_src + k0, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) u = fmaf(q[e], ra[e], u);
        }
        __syncthreads();
        if (k0 + GC_K < C) fetch(k0 + GC_K);          // next step's operands in flight under this step's MFMAs
        const float* pa = sP + (wn * 32 + l31) * GC_LD + h;
        const float* pb = sA + (wm * 32 + l31) * GC_LD + h;
#pragma unroll
        for (int kk = 0; kk < GC_K; kk += 2)          // A operand: targets (MFMA rows), B operand: map rows (MFMA columns)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
    }
    // U of row si: the 4 staging threads of a row are adjacent lanes
    u += __shfl_xor(u, 1, 64);
    u += __shfl_xor(u, 2, 64);
    if ((tid & 3) == 0) sU[si] = u;
    __syncthreads();

    // this lane: map row wm * 32 + l31 (the accumulator's column), targets wn * 32 + (e & 3) + 8 (e >> 2) + 4 h
    const int jr = wm * 32 + l31;
    const long r = r0 + jr;
    if (r >= rows_end) return;
    const int n = (int)(r / HW), p = (int)(r - (long)n * HW);
    const float U = sU[jr];
    float scale, su = 0.f;
    bool use_s = false;
    if (norm) {
        const float nr = norm[n];
        use_s = !(nr < eps);                          // F.normalize backward: (t - s n^) / ||f||, or t / eps below eps
        scale = 1.f / ((use_s ? nr : eps) * (float)HW);
        su = U;
    } else {
        scale = 1.f / (float)HW;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = c0 + wn * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (c >= cnt) continue;
        const int t = target_of(n, c);
        float v = acc[e];
        if (use_s) v = v - S[(long)n * M + t] * su;
        v *= scale;
        const long o = all ? ((long)n * M + c) * HW + p : (mode == CVCL_GRADCAM_BLOCK_IMAGE ? ((long)n * k + c) * HW + p : r);
        cam[o] = v < 0.f ? 0.f : v;                   // torch.clamp(min=0): NaN stays NaN
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// F.interpolate(x, (H, W), mode='bicubic', align_corners=False) of [maps, h, w] fp32: torch's source index
// (dst + 0.5) * in / out - 0.5 (not clamped), floor clamped to in - 1, fraction clamped to [0, 1], 4 taps clamped to the image,
// cubic convolution with A = -0.75.  A workgroup writes RPW whole output rows of one map: the 4-tap vertical blend of the rows it
// needs goes to LDS first (w values per output row), then each thread keeps the horizontal weights of its 4 output columns in
// registers for all the rows and writes them with 16-byte stores.  Write-bound.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int BIC_LDS = 4096;                         // floats of vertical blends per workgroup (w <= 4096)

__device__ __forceinline__ void cubic_weights(float scale, int dst, int in, int (&idx)[4], float (&wt)[4]) {
    const float src = scale * ((float)dst + 0.5f) - 0.5f;
    int i0 = (int)floorf(src);
    i0 = i0 < in - 1 ? i0 : in - 1;
    float t = src - (float)i0;
    t = fminf(fmaxf(t, 0.f), 1.f);
    constexpr float A = -0.75f;
    auto c1 = [](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };             // |x| <= 1
    auto c2 = [](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };      // 1 < |x| < 2
    wt[0] = c2(t + 1.f);
    wt[1] = c1(t);
    wt[2] = c1(1.f - t);
    wt[3] = c2(2.f - t);
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = min(max(i0 - 1 + j, 0), in - 1);
}

__global__ __launch_bounds__(256) void bicubic_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int H, int W,
                                                      int rpw, int tiles_per_map) {
    __shared__ float blend[BIC_LDS];
    const int map = blockIdx.x / tiles_per_map;
    const int y0 = (blockIdx.x % tiles_per_map) * rpw;
    const int rows = min(rpw, H - y0);
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const float* src = x + (long)map * h * w;
    // vertical pass: blend[r][xi] = sum_i wy_i src[yi_i][xi]
    for (int e = threadIdx.x; e < rows * w; e += blockDim.x) {
        const int r = e / w, xi = e - r * w;
        int iy[4];
        float wy[4];
        cubic_weights(sy, y0 + r, h, iy, wy);
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) v = fmaf(wy[i], src[(long)iy[i] * w + xi], v);
        blend[r * w + xi] = v;
    }
    __syncthreads();
    float* dst = y + ((long)map * H + y0) * W;
    const int G = (W + 3) / 4;                        // 4-column groups of a row
    const int nph = G >= 256 ? 1 : 256 / G;           // rows written side by side
    const int ph = G >= 256 ? 0 : threadIdx.x / G;
    if (ph >= nph) return;
    const bool vec = (W & 3) == 0;
    for (int g = G >= 256 ? threadIdx.x : threadIdx.x % G; g < G; g += G >= 256 ? 256 : G) {
        int ix[4][4];
        float wx[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cubic_weights(sx, min(4 * g + q, W - 1), w, ix[q], wx[q]);
        for (int r = ph; r < rows; r += nph) {
            const float* b = blend + r * w;
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) v = fmaf(wx[q][j], b[ix[q][j]], v);
                o[q] = v;
            }
            float* d = dst + (long)r * W + 4 * g;
            if (vec) {
                stream_store(o, reinterpret_cast<f32x4*>(d));
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (4 * g + q < W) d[q] = o[q];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gradCAM_with_act_and_grad (reference attention_maps.py:112-122): alpha[c] = mean_p grad[n, c, p], cam[n, p] = relu(sum_c alpha[c]
// act[n, c, p]).  One workgroup per image; act and grad each fp32 or bf16, each NCHW-contiguous or NHWC (channels-last) storage.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int AG_MAXC = 8192;

template <typename TA, typename TG>
__global__ __launch_bounds__(256) void act_grad_kernel(const TA* __restrict__ act, int act_nhwc, const TG* __restrict__ grad,
                                                       int grad_nhwc, float* __restrict__ cam, int C, int HW) {
    __shared__ float alpha[AG_MAXC];
    const int n = blockIdx.x;
    const long base = (long)n * C * HW;
    const long gsc = grad_nhwc ? 1 : HW, gsp = grad_nhwc ? C : 1;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += ElemTraits<TG>::to_f(grad[base + c * gsc + p * gsp]);
        alpha[c] = s / (float)HW;
    }
    __syncthreads();
    const long asc = act_nhwc ? 1 : HW, asp = act_nhwc ? C : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < HW; p += blockDim.x >> 6) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(alpha[c], ElemTraits<TA>::to_f(act[base + c * asc + p * asp]), s);
        s = wave_sum(s);
        if (lane == 0) cam[(long)n * HW + p] = s < 0.f ? 0.f : s;
    }
}

}  // namespace

extern "C" int cvcl_gradcam_pairs(int dtype, const void* map, int N, int HW, int C, const float* P, int M, int mode, int k,
                                  const float* Q, const float* S, const float* norm, float eps, float* cam, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_gradcam_pairs");
    CVCL_CHECK_ARG(map && P && cam, "cvcl_gradcam_pairs: null map / P / cam");
    CVCL_CHECK_ARG(N > 0 && HW > 0 && C > 0 && M > 0, "cvcl_gradcam_pairs: sizes must be positive (N %d HW %d C %d M %d)", N, HW, C, M);
    CVCL_CHECK_ARG(C % GC_K == 0, "cvcl_gradcam_pairs: C = %d is not a multiple of %d", C, GC_K);
    CVCL_CHECK_ARG((Q && S && norm) || (!Q && !S && !norm), "cvcl_gradcam_pairs: Q, s and norm go together (normalised features) or not at all");
    CVCL_CHECK_ARG(!norm || eps > 0.f, "cvcl_gradcam_pairs: eps must be positive");
    CVCL_CHECK_ARG(cvcl_aligned16(map) && cvcl_aligned16(P) && (!Q || cvcl_aligned16(Q)), "cvcl_gradcam_pairs: map / P / Q must be 16-byte aligned");
    if (mode == CVCL_GRADCAM_ALL) {
        CVCL_CHECK_ARG(k == 0, "cvcl_gradcam_pairs: all pairs takes k = 0 (got %d)", k);
    } else if (mode == CVCL_GRADCAM_BLOCK_IMAGE) {
        CVCL_CHECK_ARG(k > 0 && (long)N * k == M, "cvcl_gradcam_pairs: block (image) needs M = N k (N %d k %d M %d)", N, k, M);
    } else if (mode == CVCL_GRADCAM_BLOCK_TEXT) {
        CVCL_CHECK_ARG(k > 0 && (long)M * k == N, "cvcl_gradcam_pairs: block (text) needs N = M k (N %d k %d M %d)", N, k, M);
    } else {
        CVCL_CHECK_ARG(false, "cvcl_gradcam_pairs: unknown mode %d", mode);
    }
    const int rtpi = cvcl_div_up(HW, GC_TILE);
    const long row_tiles = mode == CVCL_GRADCAM_ALL ? (long)cvcl_div_up((long)N * HW, GC_TILE) : (long)N * rtpi;
    const int cnt = mode == CVCL_GRADCAM_ALL ? M : (mode == CVCL_GRADCAM_BLOCK_IMAGE ? k : 1);
    CVCL_CHECK_ARG(row_tiles <= 65535, "cvcl_gradcam_pairs: %ld row tiles exceed the grid (N HW too large)", row_tiles);
    const dim3 grid(cvcl_div_up(cnt, GC_TILE), (unsigned)row_tiles);
    CvclProfScope prof(stream, CVCL_K_HEAD);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(gradcam_pairs_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)map, N, HW, C, P, M, mode, k,
                           Q, S, norm, eps, cam, rtpi);
    else
        hipLaunchKernelGGL(gradcam_pairs_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)map, N, HW, C, P, M, mode,
                           k, Q, S, norm, eps, cam, rtpi);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_bicubic_resize(const float* x, float* y, int maps, int h, int w, int H, int W, void* stream) {
    CVCL_CHECK_ARG(x && y, "cvcl_bicubic_resize: null input / output");
    CVCL_CHECK_ARG(maps > 0 && h > 0 && w > 0 && H > 0 && W > 0, "cvcl_bicubic_resize: sizes must be positive (maps %d %dx%d -> %dx%d)",
                   maps, h, w, H, W);
    CVCL_CHECK_ARG(w <= BIC_LDS, "cvcl_bicubic_resize: input width %d > %d", w, BIC_LDS);
    CVCL_CHECK_ARG(cvcl_aligned16(y), "cvcl_bicubic_resize: output must be 16-byte aligned");
    const int rpw = max(1, min(16, BIC_LDS / w));
    const int tpm = cvcl_div_up(H, rpw);
    CVCL_CHECK_ARG((long)maps * tpm <= 0x7fffffffL, "cvcl_bicubic_resize: grid too large");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(bicubic_kernel, dim3((unsigned)(maps * tpm)), dim3(256), 0, (hipStream_t)stream, x, y, h, w, H, W, rpw, tpm);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_gradcam_act_grad(int act_dtype, const void* act, int act_nhwc, int grad_dtype, const void* grad, int grad_nhwc,
                                     float* cam, int N, int C, int HW, void* stream) {
    CVCL_CHECK_DTYPE(act_dtype, "cvcl_gradcam_act_grad");
    CVCL_CHECK_DTYPE(grad_dtype, "cvcl_gradcam_act_grad");
    CVCL_CHECK_ARG(act && grad && cam, "cvcl_gradcam_act_grad: null act / grad / cam");
    CVCL_CHECK_ARG(N > 0 && C > 0 && HW > 0, "cvcl_gradcam_act_grad: sizes must be positive (N %d C %d HW %d)", N, C, HW);
    CVCL_CHECK_ARG(C <= AG_MAXC, "cvcl_gradcam_act_grad: C = %d > %d", C, AG_MAXC);
    CVCL_CHECK_ARG((act_dtype == CVCL_F32 || act_dtype == CVCL_BF16) && (grad_dtype == CVCL_F32 || grad_dtype == CVCL_BF16),
                   "cvcl_gradcam_act_grad: dtypes %d / %d", act_dtype, grad_dtype);
    const hipStream_t s = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_OTHER);
#define CVCL_AG(TA, TG) hipLaunchKernelGGL((act_grad_kernel<TA, TG>), dim3(N), dim3(256), 0, s, (const TA*)act, act_nhwc, (const TG*)grad, \
                                           grad_nhwc, cam, C, HW)
    if (act_dtype == CVCL_F32) {
        if (grad_dtype == CVCL_F32) CVCL_AG(float, float);
        else CVCL_AG(float, bf16_t);
    } else {
        if (grad_dtype == CVCL_F32) CVCL_AG(bf16_t, float);
        else CVCL_AG(bf16_t, bf16_t);
    }
#undef CVCL_AG
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
