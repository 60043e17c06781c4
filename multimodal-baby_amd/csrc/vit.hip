// Transformer-side kernels of the DINO ViT image encoder (reference multimodal/vision_transformer_dino_mugs.py:87-250).  Every
// linear layer runs on the MFMA GEMM of gemm.hip; this file holds what is not a GEMM: patch gather, token assembly, the LayerNorm
// forwards, row statistics and the attention forwards (the generic one also serves the one-layer text transformer,
// multimodal/multimodal.py:553-573).  The text encoders' own kernels are in text.hip and lstm.hip.
#include "cvcl_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// PatchEmbed conv (k = s = p) as unfold + GEMM (vit:162,166): cols[b*np + i][c*p*p + ky*p + kx], zero padded to Kpad
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void im2col_patches_kernel(const float* __restrict__ x, T* __restrict__ cols, int B, int H,
                                                             int W, int p, int Kpad) {
    const int gh = H / p, gw = W / p, K = 3 * p * p;
    const long total = (long)B * gh * gw * Kpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kpad);
        const long r = i / Kpad;
        float v = 0.f;
        if (k < K) {
            const int c = k / (p * p), rem = k - c * p * p, ky = rem / p, kx = rem - ky * p;
            const int px = (int)(r % gw), py = (int)((r / gw) % gh), b = (int)(r / ((long)gw * gh));
            v = x[(((long)b * 3 + c) * H + py * p + ky) * W + px * p + kx];
        }
        cols[i] = ElemTraits<T>::from_f(v);
    }
}

// bf16, patch % 8 == 0 (ViT-B/16): a thread converts 8 consecutive kx of one (patch row, channel, ky) -- 32 contiguous bytes of
// the image in, 16 bytes out; index arithmetic once per 8 elements (the element-per-thread form above ran at a quarter of the
// HBM rate: 190 us for the 231 MB of a B = 256 batch)
__global__ __launch_bounds__(256) void im2col_patches8_kernel(const float* __restrict__ x, bf16_t* __restrict__ cols, int B, int H,
                                                              int W, int p, int Kpad) {
    const int gh = H / p, gw = W / p, K = 3 * p * p, cpr = Kpad / 8, ppc = p / 8;     // chunks per row / per patch line
    const long total = (long)B * gh * gw * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i % cpr);
        const long r = i / cpr;
        u32x4 o = {0u, 0u, 0u, 0u};
        if (q * 8 < K) {
            const int line = q / ppc, kx = (q - line * ppc) * 8, c = line / p, ky = line - c * p;
            const int px = (int)(r % gw), py = (int)((r / gw) % gh), b = (int)(r / ((long)gw * gh));
            const float* src = x + (((long)b * 3 + c) * H + py * p + ky) * W + px * p + kx;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
            o = u32x4{round2(f32x2{v0[0], v0[1]}), round2(f32x2{v0[2], v0[3]}), round2(f32x2{v1[0], v1[1]}), round2(f32x2{v1[2], v1[3]})};
        }
        *reinterpret_cast<u32x4*>(cols + i * 8) = o;
    }
}

// bf16, D % 8 == 0: 8 channels per thread (the element-per-thread form below: 129 us for 155 MB)
__global__ __launch_bounds__(256) void vit_assemble8_kernel(const bf16_t* __restrict__ tok, const float* __restrict__ cls,
                                                            const float* __restrict__ pos, bf16_t* __restrict__ h, int B, int Tn,
                                                            int D) {
    const int cpr = D / 8;
    const long total = (long)B * Tn * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i % cpr) * 8;
        const long r = i / cpr;
        const int t = (int)(r % Tn);
        const long b = r / Tn;
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(pos + (long)t * D + d), p1 = *reinterpret_cast<const f32x4*>(pos + (long)t * D + d + 4);
        f32x2 v[4];
        if (t == 0) {
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(cls + d), c1 = *reinterpret_cast<const f32x4*>(cls + d + 4);
            v[0] = f32x2{c0[0], c0[1]}; v[1] = f32x2{c0[2], c0[3]}; v[2] = f32x2{c1[0], c1[1]}; v[3] = f32x2{c1[2], c1[3]};
        } else {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(tok + (b * (Tn - 1) + (t - 1)) * D + d);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = widen2(raw[e]);
        }
        const u32x4 o = {round2(v[0] + f32x2{p0[0], p0[1]}), round2(v[1] + f32x2{p0[2], p0[3]}), round2(v[2] + f32x2{p1[0], p1[1]}),
                         round2(v[3] + f32x2{p1[2], p1[3]})};
        *reinterpret_cast<u32x4*>(h + i * 8) = o;
    }
}

// h[b][0] = cls + pos[0];  h[b][1+i] = tok[b][i] + pos[1+i]      (prepare_tokens, vit:232-243)
template <typename T>
__global__ __launch_bounds__(256) void vit_assemble_kernel(const T* __restrict__ tok, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, T* __restrict__ h, int B, int Tn,
                                                           int D) {
    const long total = (long)B * Tn * D;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const long r = i / D;
        const int t = (int)(r % Tn);
        const long b = r / Tn;
        const float base = t == 0 ? cls[d] : ElemTraits<T>::to_f(tok[(b * (Tn - 1) + (t - 1)) * D + d]);
        h[i] = ElemTraits<T>::from_f(base + pos[(long)t * D + d]);
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm over the last dimension, one wave per row; rows may be strided (cls-token rows); output T or fp32
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, long x_row_stride, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, TO* __restrict__ y,
                                                        long rows, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T* xr = x + row * x_row_stride;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += ElemTraits<T>::to_f(xr[d]);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float c = ElemTraits<T>::to_f(xr[d]) - mean;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int d = lane; d < D; d += 64) {
        const float v = (ElemTraits<T>::to_f(xr[d]) - mean) * rstd * gamma[d] + beta[d];
        y[row * D + d] = ElemTraits<TO>::from_f(v);
    }
}

// bf16 rows held in registers: one wave per row, up to 4 chunks of 16 B per lane (D <= 2048, D % 8 == 0, 16-byte aligned
// rows); the row is read once (the scalar kernel above walks it three times with 2-byte loads)
template <typename TO>
__global__ __launch_bounds__(256) void layernorm_bf16_vec_kernel(const bf16_t* __restrict__ x, long x_row_stride,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float eps, TO* __restrict__ y, long rows, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bf16_t* xr = x + row * x_row_stride;
    const int nch = D >> 3;
    bf16x8 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            v[i] = *reinterpret_cast<const bf16x8*>(xr + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += (float)v[i][e];
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float c = (float)v[i][e] - mean; q = fmaf(c, c, q); }
        }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + c * 8 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c * 8), b1 = *reinterpret_cast<const f32x4*>(beta + c * 8 + 4);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = ((float)v[i][e] - mean) * rstd * (e < 4 ? g0[e] : g1[e - 4]) + (e < 4 ? b0[e] : b1[e - 4]);
            if constexpr (sizeof(TO) == 2) {
                bf16x8 ov;
#pragma unroll
                for (int e = 0; e < 8; ++e) ov[e] = (bf16_t)o[e];
                *reinterpret_cast<bf16x8*>(y + row * D + c * 8) = ov;
            } else {
                *reinterpret_cast<f32x4*>(y + row * D + c * 8) = f32x4{o[0], o[1], o[2], o[3]};
                *reinterpret_cast<f32x4*>(y + row * D + c * 8 + 4) = f32x4{o[4], o[5], o[6], o[7]};
            }
        }
    }
}

// 32 lanes per row, NCH chunks of 16 B per lane (D <= 256 NCH: a 768-wide ViT-B row is exactly 3 chunks per lane, no idle lanes;
// the wave-per-row kernel above leaves half the lanes with one chunk fewer), reductions by DPP inside a 16-lane row plus one
// shuffle across (5 ds_bpermute round trips less per reduction)
__device__ inline float ln_row32_sum(float v) {
    auto dpp = [](float x, int sel) {
        const int xi = __builtin_bit_cast(int, x);
        int r;
        if (sel == 0) r = __builtin_amdgcn_update_dpp(0, xi, 0xB1, 0xf, 0xf, true);
        else if (sel == 1) r = __builtin_amdgcn_update_dpp(0, xi, 0x4E, 0xf, 0xf, true);
        else if (sel == 2) r = __builtin_amdgcn_update_dpp(0, xi, 0x141, 0xf, 0xf, true);
        else r = __builtin_amdgcn_update_dpp(0, xi, 0x140, 0xf, 0xf, true);
        return __builtin_bit_cast(float, r);
    };
    v += dpp(v, 0); v += dpp(v, 1); v += dpp(v, 2); v += dpp(v, 3);
    return v + __shfl_xor(v, 16, 64);
}
// EXACT: D == 256 NCH, every chunk exists -- no branch around the loads (a branch costs a serializing vmcnt(0) per chunk)
template <typename TO, int NCH, bool EXACT>
__global__ __launch_bounds__(256) void layernorm_bf16_row32_kernel(const bf16_t* __restrict__ x, long x_row_stride,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float eps, TO* __restrict__ y, long rows, int D) {
    const long row = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int lane = threadIdx.x & 31;
    if (row >= rows) return;
    const bf16_t* xr = x + row * x_row_stride;
    const int nch = D >> 3;
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 32 * i;
        if (EXACT || c < nch) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(xr + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = (float)a[e]; s += v[i][e]; }
        }
    }
    const float mean = ln_row32_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (EXACT || lane + 32 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float c = v[i][e] - mean; v[i][e] = c; q = fmaf(c, c, q); }
        }
    const float rstd = 1.f / sqrtf(ln_row32_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 32 * i;
        if (EXACT || c < nch) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + c * 8 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c * 8), b1 = *reinterpret_cast<const f32x4*>(beta + c * 8 + 4);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = v[i][e] * rstd * (e < 4 ? g0[e] : g1[e - 4]) + (e < 4 ? b0[e] : b1[e - 4]);
            if constexpr (sizeof(TO) == 2) {
                bf16x8 ov;
#pragma unroll
                for (int e = 0; e < 8; ++e) ov[e] = (bf16_t)o[e];
                *reinterpret_cast<bf16x8*>(y + row * D + c * 8) = ov;
            } else {
                *reinterpret_cast<f32x4*>(y + row * D + c * 8) = f32x4{o[0], o[1], o[2], o[3]};
                *reinterpret_cast<f32x4*>(y + row * D + c * 8 + 4) = f32x4{o[4], o[5], o[6], o[7]};
            }
        }
    }
}

// ---- LayerNorm folded into the consuming linear (gemm8w_kernel.h LNF): only the row statistics are computed here -----------
// out[row] = (rstd, -mean rstd).  One 32-lane group per row, the row in registers (as layernorm_bf16_row32_kernel), centred
// second moment; bf16 rows, D % 8 == 0, D <= 1024.
template <int NCH>
__global__ __launch_bounds__(256) void row_stats_bf16_kernel(const bf16_t* __restrict__ x, long x_row_stride, float* __restrict__ out,
                                                             long rows, int D, float eps) {
    const long row = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int lane = threadIdx.x & 31;
    if (row >= rows) return;
    const bf16_t* xr = x + row * x_row_stride;
    const int nch = D >> 3;
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 32 * i;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        if (c < nch) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(xr + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = (float)a[e]; s += v[i][e]; }
        }
    }
    const float mean = ln_row32_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (lane + 32 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float c = v[i][e] - mean; q = fmaf(c, c, q); }
        }
    const float rstd = 1.f / sqrtf(ln_row32_sum(q) / (float)D + eps);
    if (lane == 0) *reinterpret_cast<f32x2*>(out + row * 2) = f32x2{rstd, -mean * rstd};
}
// the producer GEMM's strip partials [rows][strips][2] (sum, sum of squares of 64 stored values each) -> (rstd, -mean rstd);
// one thread per row, fixed order, fp64 combination (E[x^2] - mean^2 on fp32 sums of exact bf16 products)
__global__ __launch_bounds__(256) void row_stats_finalize_kernel(const float* __restrict__ part, int strips, float* __restrict__ out,
                                                                 long rows, int D, float eps) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const f32x2* p = reinterpret_cast<const f32x2*>(part) + row * strips;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < strips; ++i) { const f32x2 v = p[i]; s1 += (double)v[0]; s2 += (double)v[1]; }
    const double mean = s1 / D;
    double var = s2 / D - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    *reinterpret_cast<f32x2*>(out + row * 2) = f32x2{(float)rstd, (float)(-mean * rstd)};
}

// ------------------------------------------------------------------------------------------------
// Attention, generic (any head_dim <= 128, any T, optional key padding mask): one wave per (b, head, query).
// qkv [B, T, 3, heads, hd] -> out [B, T, heads*hd].  P is rounded to the storage type before P.V.
// CAUSAL (cvcl_attention_causal, the CLIP text tower): query t walks keys 0..t only -- the masked products are never formed.
// ------------------------------------------------------------------------------------------------
template <typename T, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attention_valu_kernel(const T* __restrict__ qkv, const int64_t* __restrict__ key_tok,
                                                             T* __restrict__ out, int B, int Tn, int heads, int hd,
                                                             float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* sq = (float*)smem + (size_t)wave * (hd + Tn);     // q vector then probabilities, per wave
    float* sp = sq + hd;
    const long widx = (long)blockIdx.x * 4 + wave;
    const long nwork = (long)B * heads * Tn;
    if (widx >= nwork) return;
    const int qi = (int)(widx % Tn), hh = (int)((widx / Tn) % heads), b = (int)(widx / ((long)Tn * heads));
    const int D = heads * hd;
    const T* base = qkv + (long)b * Tn * 3 * D;
    const T* qp = base + (long)qi * 3 * D + hh * hd;
    const int Tk = CAUSAL ? qi + 1 : Tn;                     // keys this query attends to
    for (int d = lane; d < hd; d += 64) sq[d] = ElemTraits<T>::to_f(qp[d]);
    float mx = -INFINITY;
    for (int j = lane; j < Tk; j += 64) {
        const T* kp = base + (long)j * 3 * D + D + hh * hd;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(sq[d], ElemTraits<T>::to_f(kp[d]), s);
        s *= scale;
        if (key_tok && key_tok[(long)b * Tn + j] == 0) s = -INFINITY;     // src_key_padding_mask (x == 0)
        sp[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < Tk; j += 64) {
        const float e = expf(sp[j] - mx);
        sp[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    for (int j = lane; j < Tk; j += 64) sp[j] = ElemTraits<T>::to_f(ElemTraits<T>::from_f(sp[j] / sum));
    T* op = out + ((long)b * Tn + qi) * D + hh * hd;
    for (int d = lane; d < hd; d += 64) {
        float acc = 0.f;
        for (int j = 0; j < Tk; ++j) acc = fmaf(sp[j], ElemTraits<T>::to_f(base[(long)j * 3 * D + 2 * D + hh * hd + d]), acc);
        op[d] = ElemTraits<T>::from_f(acc);
    }
}

// ------------------------------------------------------------------------------------------------
// Attention, bf16 MFMA, head_dim 64 (ViT-B: 12 x 64): ONE workgroup per (image, head) -- K and V of the head are staged
// into LDS once (coalesced 16-byte rows, no transposed copy) and every wave walks 16-query tiles over them:
//   S^T = K Q^T   v_mfma_f32_16x16x32_bf16, A = K rows from LDS (ds_read_b128, pitch 144 B), B = Q^T from global
//   softmax       in registers (a lane holds 4 keys of every 16-key tile for one query; 2 shuffles finish the row)
//   O = P V       P goes through a wave-private LDS strip into the A layout; the B operand needs 8 keys of one d per
//                 lane, i.e. the transpose of the row-major V image: gfx950 ds_read_b64_tr_b16 (pitch 160 B keeps the
//                 8 rows x 32 B that 32 lanes touch on disjoint banks).  The k index of a lane's block is
//                 {32ks + 4g + e} U {32ks + 16 + 4g + e} in BOTH operands (any fixed permutation of k is valid).
//   out           staged through the P strip, written as 16-byte row pieces.
// (The first version ran one workgroup per 64 queries: V^T was rebuilt 4x per head with 2-byte LDS scatters, 4-way
//  bank conflicted, and K was re-read from L2 by every wave: 440 us per ViT-B/16 layer at B = 256.)
// ------------------------------------------------------------------------------------------------
constexpr int ATT_TPAD_MAX = 288;      // keys padded to a multiple of 32 (T <= 288 covers ViT-B/14 at 224: 257)
constexpr int ATT_THREADS = 512;       // 8 waves: the 7 query tiles of a 197-token ViT-B/16 head run in ONE round (4 waves needed two, the
                                       // second half empty), two workgroups per CU = 4 waves per SIMD
constexpr int ATT_STAGE_IT = (ATT_TPAD_MAX * 8 + ATT_THREADS - 1) / ATT_THREADS;   // staging chunks per thread (5 at 288 rows)
constexpr int ATT_KP = 144;            // LDS bytes per K row (128 + 16)
constexpr int ATT_VP = 192;            // LDS bytes per V row (128 + 64): the 4 rows x 64 B that 32 lanes touch in one
                                       // ds_read_b64_tr_b16 land on banks 0-15 / 48-63 / 32-47 / 16-31

typedef __bf16 att_tr4 __attribute__((__vector_size__(4 * sizeof(__bf16))));
__device__ inline bf16x4 att_tr_read(const char* p) {
    auto lp = reinterpret_cast<__attribute__((address_space(3))) att_tr4*>((__attribute__((address_space(3))) char*)(p));
    return __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4bf16(lp));
}

// One workgroup (4 waves) per (image, head); K and V of the head are staged into LDS once (row-major, coalesced); every
// wave walks 32-query tiles, streaming over 32-key tiles with an online softmax (running max / sum per query):
//   S^T = K Q^T     v_mfma_f32_32x32x16_bf16, A = K rows from LDS (ds_read_b128), B = Q^T fragments from global; a lane
//                   ends up with 16 of the 32 keys of the tile for ONE query (its column l31): keys 8b + 4h + c
//   softmax         in registers: the lane's query statistics are shared only with lane ^ 32
//   O^T += V^T P^T  P never leaves the registers: the 8 probabilities a lane holds for a 16-key step (keys 16u + 4h + c
//                   and 16u + 8 + 4h + c) ARE a valid B-operand k block for its query, provided the A operand uses the
//                   same key assignment -- V^T fragments (8 keys of one d per lane = the transpose of the row-major
//                   image) come from two ds_read_b64_tr_b16 at key offsets 4h and 8 + 4h.  O^T keeps the query in the
//                   lane's column, so the running rescale is one multiplier per lane.
//   LDS = Tpad * 336 B (75 KB at T = 197): two workgroups per CU, so one stages while the other multiplies.
// (v1: one workgroup per 64 queries, V^T rebuilt with 2-byte scatters: 440 us per ViT-B/16 layer at B = 256;
//  v2: per-head workgroup, 16-query tiles, all of S in registers, P through LDS, 1 workgroup/CU: 190 us.)
// MX = true: the output is written as e4m3 with one e8m0 scale per (row, 32 d) instead of bf16 (cvcl_gemm_fp8_mx's input format:
// bytes [B*T][D], scales tiled [D/128][B*T][4]) -- a lane and its partner lane ^ 32 hold the 32 d of one block of one query.
// NTC > 0 (round 4): the number of 32-key tiles is the compile-time NTC (9: ViT patch 14 at 224 x 224, 257 tokens) and the softmax
// is TWO-PASS: all NTC score tiles of a query tile stay in registers (16 NTC accumulators), the row maximum
// is taken once, then every tile is exponentiated and multiplied with V -- no running maximum, no rescale of O: ~50 VALU
// instructions per key tile instead of ~100 in a loop that is VALU-issue-bound (profiles/r04_pmc_c4_summary.txt: 17.8 VALU
// instructions per MFMA, matrix pipe 19 % busy).  NTC = 0: the online-softmax loop for any other token count.
template <bool MX, int NTC>
__global__ __launch_bounds__(ATT_THREADS, 2) void attention_mfma_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                unsigned char* __restrict__ out8, unsigned char* __restrict__ out_bs,
                                                                float* __restrict__ lse, int B, int Tn, int heads, float scale, int NT) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Tpad = 32 * NT;
    char* sK = smem;                                                // [Tpad][ATT_KP]
    char* sV = sK + Tpad * ATT_KP;                                  // [Tpad][ATT_VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int hh = blockIdx.x % heads, b = blockIdx.x / heads;
    const int D = heads * 64;
    const bf16_t* base = qkv + (long)b * Tn * 3 * D;

    // K and V rows -> LDS, 8 chunks of 16 B per row, zeros beyond Tn.  All of a thread's loads (<= ATT_STAGE_IT pairs) are issued
    // before the first LDS write: the plain loop waited for each pair (a dependent L2 round trip per iteration, ~half of the
    // workgroup's lifetime at 197 tokens)
    u32x4 kv[ATT_STAGE_IT], vv[ATT_STAGE_IT];
#pragma unroll
    for (int it = 0; it < ATT_STAGE_IT; ++it) {
        const int i = tid + it * ATT_THREADS;
        const int jc = min(i >> 3, Tn - 1), c = i & 7;                       // clamped row: always a valid address, no branch
        kv[it] = *reinterpret_cast<const u32x4*>(base + (long)jc * 3 * D + D + hh * 64 + c * 8);
        vv[it] = *reinterpret_cast<const u32x4*>(base + (long)jc * 3 * D + 2 * D + hh * 64 + c * 8);
    }
#pragma unroll
    for (int it = 0; it < ATT_STAGE_IT; ++it) {
        const int i = tid + it * ATT_THREADS;
        const int j = i >> 3, c = i & 7;
        if (i < Tpad * 8) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(sK + j * ATT_KP + c * 16) = j < Tn ? kv[it] : z;
            *reinterpret_cast<u32x4*>(sV + j * ATT_VP + c * 16) = j < Tn ? vv[it] : z;
        }
    }
    __syncthreads();

    const float scale2 = scale * 1.4426950408889634f;               // logits in units of log2(e): exp(x) = 2^(x log2 e)
    const int nqt = (Tn + 31) / 32;
    // tr-read addressing inside a [4 keys][16 d] block: 16-lane group (lane >> 4) & 1 takes d columns +16
    const int l15 = lane & 15;
    const int v_lane_off = (4 * h + (l15 >> 2)) * ATT_VP + (((lane >> 4) & 1) * 16 + (l15 & 3) * 4) * 2;

    for (int qt = wave; qt < nqt; qt += ATT_THREADS / 64) {
        const int q0 = qt * 32;
        const int qrow = min(q0 + l31, Tn - 1);
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(base + (long)qrow * 3 * D + hh * 64 + ks * 16 + h * 8);

        f32x16 o[2];                                                // O^T: rows d = 32 dt + 8b + 4h + c, column = this lane's query
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;                       // l_run: this lane's share of the row sum

        if constexpr (NTC > 0) {
            // ---- two-pass form: S^T for all NTC key tiles, one row maximum, then exp + O^T += V^T P^T per tile ----
            f32x16 sc[NTC];
#pragma unroll
            for (int t = 0; t < NTC; ++t) {
#pragma unroll
                for (int e = 0; e < 16; ++e) sc[t][e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (t * 32 + l31) * ATT_KP + ks * 32 + h * 16);
                    sc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sc[t], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);                  // (tile by tile: hoisting every tile's reads spills)
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {                          // keys >= Tn exist in the last tile only
                const int key = (NTC - 1) * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                sc[NTC - 1][r] = key < Tn ? sc[NTC - 1][r] : -INFINITY;
            }
            float mx = sc[0][0];
#pragma unroll
            for (int t = 0; t < NTC; ++t)
#pragma unroll
                for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, sc[t][r]), sc[t][r + 1]);        // v_max3_f32
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            m_run = mx * scale2;                                    // finite: key 0 is always valid
            const f32x2 sc2 = {scale2, scale2}, nm2 = {-m_run, -m_run};
            f32x2 ps2 = {0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NTC; ++t) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2 a = __builtin_elementwise_fma(f32x2{sc[t][r], sc[t][r + 1]}, sc2, nm2);
                    sc[t][r] = __builtin_amdgcn_exp2f(a[0]);
                    sc[t][r + 1] = __builtin_amdgcn_exp2f(a[1]);
                    ps2 += f32x2{sc[t][r], sc[t][r + 1]};
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    bf16x8 pf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[e] = (bf16_t)sc[t][8 * u + e];
                    const char* vb = sV + (t * 32 + 16 * u) * ATT_VP + v_lane_off;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const bf16x4 v0 = att_tr_read(vb + dt * 64);
                        const bf16x4 v1 = att_tr_read(vb + 8 * ATT_VP + dt * 64);
                        const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            l_run = ps2[0] + ps2[1];
        }
        for (int t = 0; t < (NTC > 0 ? 0 : NT); ++t) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (t * 32 + l31) * ATT_KP + ks * 32 + h * 16);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
            // softmax bookkeeping is the VALU half of this loop (per 32-key tile: 16 exponentials, the running-max update and the
            // rescale of 32 accumulators against 8 MFMAs), so it is kept lean: logits stay unscaled (the scale folds into the
            // exponent's fma), keys are masked only in the last tile (the only one with keys >= Tn), arithmetic runs on register
            // pairs (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32)
            if (t == NT - 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                    acc[r] = key < Tn ? acc[r] : -INFINITY;
                }
            }
            float mx = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx * scale2);          // finite: key 0 of tile 0 is always valid (scale2 > 0)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            const f32x2 sc2 = {scale2, scale2}, nm2 = {-m_new, -m_new};
            f32x2 ps2 = {0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 a = __builtin_elementwise_fma(f32x2{acc[r], acc[r + 1]}, sc2, nm2);
                acc[r] = __builtin_amdgcn_exp2f(a[0]);              // v_exp_f32 (exp2(-inf) = 0 for the masked keys)
                acc[r + 1] = __builtin_amdgcn_exp2f(a[1]);
                ps2 += f32x2{acc[r], acc[r + 1]};
            }
            l_run = fmaf(l_run, alpha, ps2[0] + ps2[1]);
            {       // (round 5: unconditionally -- `if (__any(alpha != 1.f))` saved 16 packed multiplies on tiles where no row maximum moved,
                    //  but the branch ended a basic block in the middle of the key-tile step: 86-89 -> 85-88 us per layer; x * 1.0f keeps the bits)
                const f32x2 al2 = {alpha, alpha};
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int e = 0; e < 16; e += 2) {
                        const f32x2 v = f32x2{o[dt][e], o[dt][e + 1]} * al2;
                        o[dt][e] = v[0]; o[dt][e + 1] = v[1];
                    }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                bf16x8 pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (bf16_t)acc[8 * u + e];
                const char* vb = sV + (t * 32 + 16 * u) * ATT_VP + v_lane_off;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16x4 v0 = att_tr_read(vb + dt * 64);
                    const bf16x4 v1 = att_tr_read(vb + 8 * ATT_VP + dt * 64);
                    const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv = 1.f / l_tot;
        // log-sum-exp of the row's logits in log2 units (what the backward kernels rebuild the probabilities from)
        if (lse && h == 0 && q0 + l31 < Tn) lse[((long)b * heads + hh) * Tn + q0 + l31] = m_run + log2f(l_tot);
        // this lane's query row: 8 runs of 4 consecutive d (d = 32 dt + 8b + 4h + c)
        if constexpr (MX) {
            const long mrow = (long)b * Tn + q0 + l31, Mtot = (long)B * Tn;
            unsigned sbs[2];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                float vq[16], amax = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) { vq[e] = (float)(bf16_t)(o[dt][e] * inv); amax = fmaxf(amax, fabsf(vq[e])); }   // as the bf16 output
                amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
                sbs[dt] = mx_scale_byte(amax);
                const float qi = mx_inv_scale(sbs[dt]);
                // (the same lane-pair exchange as the bf16 output below: 8-byte pieces instead of 4-byte ones)
                unsigned w[4];
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) w[bb] = pack4_fp8(vq[4 * bb] * qi, vq[4 * bb + 1] * qi, vq[4 * bb + 2] * qi, vq[4 * bb + 3] * qi);
                const auto s01 = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);
                const auto s23 = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);
                if (q0 + l31 < Tn) {
                    unsigned char* dst = out8 + mrow * D + hh * 64 + dt * 32 + 8 * h;
                    *reinterpret_cast<u32x2*>(dst) = u32x2{s01[0], s01[1]};
                    *reinterpret_cast<u32x2*>(dst + 16) = u32x2{s23[0], s23[1]};
                }
            }
            if (q0 + l31 < Tn && h == 0)                           // d blocks 2 hh, 2 hh + 1 of tile hh / 2
                *reinterpret_cast<unsigned short*>(out_bs + ((long)(hh >> 1) * Mtot + mrow) * 4 + 2 * (hh & 1)) =
                    (unsigned short)(sbs[0] | (sbs[1] << 8));
        } else {
            // a lane and its partner (lane ^ 32) hold alternating 4-element runs of the query's 64 d; one v_permlane32_swap per
            // register gives each of them whole 8-element runs, so the row leaves in 16-byte pieces (8 stores of 8 B before)
            const bool valid = q0 + l31 < Tn;
            bf16_t* orow = out + ((long)b * Tn + min(q0 + l31, Tn - 1)) * D + hh * 64 + 8 * h;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int e0 = 8 * j;                          // runs bb = 2 j (elements e0 .. e0+3) and 2 j + 1 (e0+4 .. e0+7)
                    const unsigned a0 = round2(f32x2{o[dt][e0 + 0] * inv, o[dt][e0 + 1] * inv});
                    const unsigned a1 = round2(f32x2{o[dt][e0 + 2] * inv, o[dt][e0 + 3] * inv});
                    const unsigned b0 = round2(f32x2{o[dt][e0 + 4] * inv, o[dt][e0 + 5] * inv});
                    const unsigned b1 = round2(f32x2{o[dt][e0 + 6] * inv, o[dt][e0 + 7] * inv});
                    const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                    const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                    if (valid) *reinterpret_cast<u32x4*>(orow + dt * 32 + 16 * j) = u32x4{s0[0], s1[0], s0[1], s1[1]};
                }
        }
    }
}

}  // namespace

// ================================================================================================
extern "C" int cvcl_im2col_patches(int dtype, const float* x_nchw, void* cols, int B, int H, int W, int patch, int Kpad,
                                   void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_im2col_patches");
    CVCL_CHECK_ARG(x_nchw && cols && B > 0 && patch > 0 && H % patch == 0 && W % patch == 0 && Kpad >= 3 * patch * patch,
                   "cvcl_im2col_patches: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const long total = (long)B * (H / patch) * (W / patch) * Kpad;
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(im2col_patches_kernel<float>, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x_nchw,
                           (float*)cols, B, H, W, patch, Kpad);
    else if (patch % 8 == 0 && Kpad % 8 == 0 && W % 4 == 0 && ((uintptr_t)x_nchw & 15) == 0 && ((uintptr_t)cols & 15) == 0)
        hipLaunchKernelGGL(im2col_patches8_kernel, dim3(cvcl_grid(total / 8, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x_nchw,
                           (bf16_t*)cols, B, H, W, patch, Kpad);
    else
        hipLaunchKernelGGL(im2col_patches_kernel<bf16_t>, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x_nchw,
                           (bf16_t*)cols, B, H, W, patch, Kpad);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_vit_assemble_tokens(int dtype, const void* tok, const float* cls, const float* pos, void* h, int B, int T,
                                        int D, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_vit_assemble_tokens");
    CVCL_CHECK_ARG(tok && cls && pos && h && B > 0 && T > 1 && D > 0, "cvcl_vit_assemble_tokens: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const long total = (long)B * T * D;
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(vit_assemble_kernel<float>, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float*)tok,
                           cls, pos, (float*)h, B, T, D);
    else if (D % 8 == 0 && ((uintptr_t)tok & 15) == 0 && ((uintptr_t)h & 15) == 0 && ((uintptr_t)pos & 15) == 0 && ((uintptr_t)cls & 15) == 0)
        hipLaunchKernelGGL(vit_assemble8_kernel, dim3(cvcl_grid(total / 8, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)tok, cls,
                           pos, (bf16_t*)h, B, T, D);
    else
        hipLaunchKernelGGL(vit_assemble_kernel<bf16_t>, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)tok, cls, pos, (bf16_t*)h, B, T, D);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_layernorm(int dtype, const void* x, long x_row_stride, const float* gamma, const float* beta, float eps,
                              void* y, int y_is_f32, long rows, int D, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_layernorm");
    CVCL_CHECK_ARG(x && gamma && beta && y && rows > 0 && D > 0 && x_row_stride >= D, "cvcl_layernorm: bad args");
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    dim3 grid(cvcl_div_up(rows, 4));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL((layernorm_kernel<float, float>), grid, dim3(256), 0, s, (const float*)x, x_row_stride, gamma, beta,
                           eps, (float*)y, rows, D);
    else {
        const bool vec = D % 8 == 0 && D <= 2048 && x_row_stride % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
                         ((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0;
        if (vec && !y_is_f32 && D <= 768 && rows >= 4096)                  // ViT-S/B token matrices
            if (D == 768)
                hipLaunchKernelGGL((layernorm_bf16_row32_kernel<bf16_t, 3, true>), dim3(cvcl_div_up(rows, 8)), dim3(256), 0, s, (const bf16_t*)x,
                                   x_row_stride, gamma, beta, eps, (bf16_t*)y, rows, D);
            else
                hipLaunchKernelGGL((layernorm_bf16_row32_kernel<bf16_t, 3, false>), dim3(cvcl_div_up(rows, 8)), dim3(256), 0, s, (const bf16_t*)x,
                                   x_row_stride, gamma, beta, eps, (bf16_t*)y, rows, D);
        else if (vec && y_is_f32)
            hipLaunchKernelGGL((layernorm_bf16_vec_kernel<float>), grid, dim3(256), 0, s, (const bf16_t*)x, x_row_stride, gamma, beta,
                               eps, (float*)y, rows, D);
        else if (vec)
            hipLaunchKernelGGL((layernorm_bf16_vec_kernel<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)x, x_row_stride, gamma, beta,
                               eps, (bf16_t*)y, rows, D);
        else if (y_is_f32)
            hipLaunchKernelGGL((layernorm_kernel<bf16_t, float>), grid, dim3(256), 0, s, (const bf16_t*)x, x_row_stride, gamma, beta,
                               eps, (float*)y, rows, D);
        else
            hipLaunchKernelGGL((layernorm_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)x, x_row_stride, gamma, beta,
                               eps, (bf16_t*)y, rows, D);
    }
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_row_stats(int dtype, const void* x, long x_row_stride, float* out, long rows, int D, float eps, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_row_stats");
    CVCL_CHECK_ARG(x && out && rows > 0 && D > 0, "cvcl_row_stats: bad args");
    CVCL_CHECK_ARG(dtype == CVCL_BF16 && D % 8 == 0 && D <= 1024 && x_row_stride % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0,
                   "cvcl_row_stats: bf16 rows with D %% 8 == 0, D <= 1024, 16-byte aligned (D %d)", D);
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    if (D <= 768)
        hipLaunchKernelGGL((row_stats_bf16_kernel<3>), dim3(cvcl_div_up(rows, 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           x_row_stride, out, rows, D, eps);
    else
        hipLaunchKernelGGL((row_stats_bf16_kernel<4>), dim3(cvcl_div_up(rows, 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           x_row_stride, out, rows, D, eps);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_row_stats_finalize(const float* row_part, int strips, float* out, long rows, int D, float eps, void* stream) {
    CVCL_CHECK_ARG(row_part && out && rows > 0 && strips > 0 && D == strips * 64 && ((uintptr_t)row_part & 7) == 0 && ((uintptr_t)out & 7) == 0,
                   "cvcl_row_stats_finalize: bad args (strips %d, D %d)", strips, D);
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    hipLaunchKernelGGL(row_stats_finalize_kernel, dim3(cvcl_div_up(rows, 256)), dim3(256), 0, (hipStream_t)stream, row_part, strips, out,
                       rows, D, eps);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

namespace {
template <bool MX, int NTC>
int launch_attention_mfma_n(const void* qkv, void* out, void* out8, void* out_bs, float* lse, int B, int T, int heads, float scale,
                            hipStream_t s) {
    const int nt = (T + 31) / 32;
    const size_t lds = (size_t)nt * 32 * (ATT_KP + ATT_VP);
    static CvclLdsAttr attr_set;
    if (const int rc = cvcl_raise_lds_limit(attr_set, (const void*)attention_mfma_kernel<MX, NTC>, 160 * 1024,
                                            "cvcl_attention"))
        return rc;
    attr_set.mark();
    hipLaunchKernelGGL((attention_mfma_kernel<MX, NTC>), dim3(B * heads), dim3(ATT_THREADS), lds, s, (const bf16_t*)qkv, (bf16_t*)out,
                       (unsigned char*)out8, (unsigned char*)out_bs, lse, B, T, heads, scale, nt);
    return CVCL_OK;
}
template <bool MX>
int launch_attention_mfma(const void* qkv, void* out, void* out8, void* out_bs, float* lse, int B, int T, int heads, float scale,
                          hipStream_t s) {
    const int nt = (T + 31) / 32;                            // the two-pass form for the token counts of ViT patch 16 / 14 at 224 x 224
    // Measured (same box, B = 256, 12 layers): 257 tokens (one workgroup per CU: 97 KB of K / V, nobody to overlap with) 2.47 -> 2.13 ms;
    // 197 tokens (two workgroups per CU overlap each other's VALU and MFMA phases) 1.23 -> 1.44 ms: the online loop stays there
    if (nt == 9) return launch_attention_mfma_n<MX, 9>(qkv, out, out8, out_bs, lse, B, T, heads, scale, s);
    return launch_attention_mfma_n<MX, 0>(qkv, out, out8, out_bs, lse, B, T, heads, scale, s);
}
}  // namespace

// bf16 qkv -> attention output as e4m3 [B*T][D] + e8m0 block scales [D/128][B*T][4] (the MX input of cvcl_gemm_fp8_mx)
extern "C" int cvcl_attention_mx(const void* qkv, void* out8, void* out_block_scales, int B, int T, int heads, int head_dim, float scale,
                                 void* stream) {
    CVCL_CHECK_ARG(qkv && out8 && out_block_scales && B > 0 && T > 0 && heads > 0, "cvcl_attention_mx: bad args");
    CVCL_CHECK_ARG(head_dim == 64 && heads % 2 == 0 && T > 32 && T <= ATT_TPAD_MAX,
                   "cvcl_attention_mx: needs head_dim 64, an even head count and 32 < T <= %d (got hd %d heads %d T %d)", ATT_TPAD_MAX, head_dim,
                   heads, T);
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    const int rc = launch_attention_mfma<true>(qkv, nullptr, out8, out_block_scales, nullptr, B, T, heads, scale, (hipStream_t)stream);
    if (rc) return rc;
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// forward for training: the bf16 MFMA kernel, additionally saving each row's log-sum-exp (log2 units) for cvcl_attention_bwd
extern "C" int cvcl_attention_train(const void* qkv, void* out, float* lse, int B, int T, int heads, int head_dim, float scale,
                                    void* stream) {
    CVCL_CHECK_ARG(qkv && out && lse && B > 0 && heads > 0, "cvcl_attention_train: bad args");
    CVCL_CHECK_ARG(head_dim == 64 && T > 32 && T <= ATT_TPAD_MAX, "cvcl_attention_train: needs head_dim 64 and 32 < T <= %d (got hd %d, T %d)",
                   ATT_TPAD_MAX, head_dim, T);
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    const int rc = launch_attention_mfma<false>(qkv, out, nullptr, nullptr, lse, B, T, heads, scale, (hipStream_t)stream);
    if (rc) return rc;
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

namespace {
template <bool CAUSAL>
int launch_attention_valu(int dtype, const void* qkv, const int64_t* key_tok, void* out, int B, int T, int heads, int head_dim, float scale,
                          hipStream_t s, const char* who) {
    const long nwork = (long)B * heads * T;
    const size_t lds = (size_t)4 * (head_dim + T) * sizeof(float);
    CVCL_CHECK_ARG(lds <= 64 * 1024, "%s: sequence too long for the generic kernel (%d)", who, T);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL((attention_valu_kernel<float, CAUSAL>), dim3(cvcl_div_up(nwork, 4)), dim3(256), lds, s, (const float*)qkv, key_tok,
                           (float*)out, B, T, heads, head_dim, scale);
    else
        hipLaunchKernelGGL((attention_valu_kernel<bf16_t, CAUSAL>), dim3(cvcl_div_up(nwork, 4)), dim3(256), lds, s, (const bf16_t*)qkv,
                           key_tok, (bf16_t*)out, B, T, heads, head_dim, scale);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
}  // namespace

extern "C" int cvcl_attention(int dtype, const void* qkv, const int64_t* key_tok, void* out, int B, int T, int heads,
                              int head_dim, float scale, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_attention");
    CVCL_CHECK_ARG(qkv && out && B > 0 && T > 0 && heads > 0 && head_dim > 0 && head_dim <= 128, "cvcl_attention: bad args");
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CVCL_BF16 && head_dim == 64 && !key_tok && T > 32 && T <= ATT_TPAD_MAX) {   // T <= 32: generic kernel below
        const int rc = launch_attention_mfma<false>(qkv, out, nullptr, nullptr, nullptr, B, T, heads, scale, s);
        if (rc) return rc;
        CVCL_LAUNCH_CHECK();
        return CVCL_OK;
    }
    return launch_attention_valu<false>(dtype, qkv, key_tok, out, B, T, heads, head_dim, scale, s, "cvcl_attention");
}

// causal self-attention of the CLIP text tower (reference eval.py:205-207, 224-226: clip's encode_text): the generic kernel for both
// storage types -- at 77 tokens the text tower is a negligible share of a CLIP pass, so the MFMA kernel has no causal form
extern "C" int cvcl_attention_causal(int dtype, const void* qkv, void* out, int B, int T, int heads, int head_dim, float scale,
                                     void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_attention_causal");
    CVCL_CHECK_ARG(qkv && out && B > 0 && T > 0 && heads > 0 && head_dim > 0 && head_dim <= 128, "cvcl_attention_causal: bad args");
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    return launch_attention_valu<true>(dtype, qkv, nullptr, out, B, T, heads, head_dim, scale, (hipStream_t)stream, "cvcl_attention_causal");
}
