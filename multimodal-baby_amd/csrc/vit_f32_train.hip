// fp32 fine-tuning of the DINO ViT (reference: vision_transformer_dino_mugs.py:87-149 Mlp / Attention / Block under autograd at
// Lightning's default precision "32"): the pieces of the fp32 trunk backward that the bf16 path has only in bf16.
//
//   attention       cvcl_attention_train_f32 (forward + log-sum-exp) and cvcl_attention_bwd_f32 (dQ kernel + dK/dV kernel), every
//                   product on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain)
//   LayerNorm       cvcl_layernorm_bwd_rows_f32 (fp32 x / dy / add / dx, dgamma / dbeta partial rows for cvcl_colsum_f32)
//   tokens          cvcl_vit_tokens_bwd_f32
//   linear          cvcl_gemm_tn_colsum_f32: dW = dY^T X and db = colsum(dY) in one pass over dY on v_mfma_f32_32x32x2_f32
//   GELU            cvcl_gelu_f32: the erff form of cvcl_gemm's fp32 GELU epilogue, and its derivative
//
// No atomics anywhere; every reduction has a fixed order: two runs are bit-identical.
//
// The attention kernels follow attention_bwd.hip's shape -- one workgroup per (image, head), the streamed operands of the head in
// LDS, a wave OWNS 32 queries (forward, dQ) or 32 keys (dK / dV) -- with the MFMA operand maps of the fp32 32x32x2 form: lane l
// supplies A[l & 31][k = l >> 5] and B[k = l >> 5][l & 31] per step, so
//   * a product over head_dim (S = Q K^T, dP = dO V^T) takes one 16-byte LDS read per lane and 4 steps: step c of chunk g contracts
//     d = 8g + c (lane half 0) and d = 8g + 4 + c (lane half 1), in both operands;
//   * a product over the 32 tokens of a tile (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS) takes the 16
//     accumulator registers of the first product AS its B operand with no lane movement: register r of lane half h holds token
//     (r & 3) + 8 (r >> 2) + 4h, so step r contracts those two tokens, and the A operand is one ds_read_b32 of that token's row.
// fp32 rows at a pitch of 68 floats (272 B: the 16-byte reads of 16 rows land on distinct banks); two operands of T <= 288 rows take
// 157 KB, i.e. one workgroup of 8 waves per CU.
#include "cvcl_common.h"

namespace {

constexpr int AF_TPAD_MAX = 288;
constexpr int AF_P = 68;                // LDS row pitch in floats
constexpr int AF_THREADS = 512;         // 8 waves: the 7 query tiles of a 197-token head in one round, 2 waves per SIMD
constexpr int AF_WAVES = AF_THREADS / 64;

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.f;
    return z;
}
// token (row of the 32-row tile) held by accumulator register r of lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// rows j < Tn of two [*, 64] fp32 matrices (row strides st0 / st1 floats) -> LDS at pitch AF_P; rows Tn .. Tpad-1 zero
__device__ inline void af_stage2(float* d0, const float* s0, long st0, float* d1, const float* s1, long st1, int Tn, int Tpad) {
    for (int i = threadIdx.x; i < Tpad * 16; i += AF_THREADS) {
        const int j = i >> 4, c = i & 15;
        const int js = min(j, Tn - 1);
        f32x4 a = *reinterpret_cast<const f32x4*>(s0 + (long)js * st0 + c * 4);
        f32x4 b = *reinterpret_cast<const f32x4*>(s1 + (long)js * st1 + c * 4);
        if (j >= Tn) a = b = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(d0 + j * AF_P + c * 4) = a;
        *reinterpret_cast<f32x4*>(d1 + j * AF_P + c * 4) = b;
    }
}

// qkv [B][T][3][heads][64] fp32 -> out [B][T][heads*64] fp32 and lse [B][heads][T] (log2 units: P = exp2(S scale log2(e) - lse)).
// Online softmax over 32-key tiles; O^T stays in registers with the query in the lane's column (one rescale factor per lane).
__global__ __launch_bounds__(AF_THREADS) void attention_f32_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                      float* __restrict__ lse, int Tn, int heads, float scale, int NT) {
    extern __shared__ __attribute__((aligned(16))) float afs[];
    const int Tpad = 32 * NT;
    float* sK = afs;
    float* sV = afs + Tpad * AF_P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int hh = blockIdx.x % heads, b = blockIdx.x / heads;
    const int D = heads * 64;
    const long rs = 3L * D;
    const float* base = qkv + (long)b * Tn * rs + hh * 64;
    af_stage2(sK, base + D, rs, sV, base + 2 * D, rs, Tn, Tpad);
    __syncthreads();
    const float scale2 = scale * 1.4426950408889634f;
    for (int qt = wave; qt < NT; qt += AF_WAVES) {
        const int q0 = qt * 32, qrow = min(q0 + l31, Tn - 1);
        f32x4 qv[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) qv[g] = *reinterpret_cast<const f32x4*>(base + (long)qrow * rs + 8 * g + 4 * h);
        float m = -INFINITY, l = 0.f;
        f32x16 o0 = zero16(), o1 = zero16();
        for (int t = 0; t < NT; ++t) {
            f32x16 s = zero16();
            const float* kr = sK + (t * 32 + l31) * AF_P + 4 * h;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(kr + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) s = mfma2(kf[c], qv[g][c], s);                 // S^T [key][query]
            }
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = t * 32 + acc_row(r, h) < Tn ? s[r] * scale2 : -INFINITY;
                mt = fmaxf(mt, s[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float mn = fmaxf(m, mt);                                                  // finite: every tile holds a key
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __builtin_amdgcn_exp2f(s[r] - mn);
                ps += s[r];
            }
            ps += __shfl_xor(ps, 32, 64);
            l = fmaf(l, alpha, ps);
            m = mn;
#pragma unroll
            for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {                                                  // O^T [d][query] += V^T P^T
                const float* vr = sV + (t * 32 + acc_row(r, h)) * AF_P + l31;
                o0 = mfma2(vr[0], s[r], o0);
                o1 = mfma2(vr[32], s[r], o1);
            }
        }
        if (q0 + l31 < Tn) {
            float* orow = out + ((long)b * Tn + q0 + l31) * D + hh * 64;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4*>(orow + 8 * g + 4 * h) = f32x4{o0[4 * g] / l, o0[4 * g + 1] / l, o0[4 * g + 2] / l, o0[4 * g + 3] / l};
                *reinterpret_cast<f32x4*>(orow + 32 + 8 * g + 4 * h) = f32x4{o1[4 * g] / l, o1[4 * g + 1] / l, o1[4 * g + 2] / l, o1[4 * g + 3] / l};
            }
            if (h == 0) lse[((long)b * heads + hh) * Tn + q0 + l31] = m + log2f(l);
        }
    }
}

// dQ: a wave owns 32 queries and streams the key tiles of K and V from LDS:  S^T = K Q^T,  dP^T = V dO^T,
// dS^T = P^T o (dP^T - D),  dQ^T += K^T dS^T;  D_q = sum_d dO O in fp32.  Writes the q third of d_qkv.
__global__ __launch_bounds__(AF_THREADS) void attention_f32_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                         const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                         float* __restrict__ d_qkv, int Tn, int heads, float scale, int NT) {
    extern __shared__ __attribute__((aligned(16))) float afs[];
    const int Tpad = 32 * NT;
    float* sK = afs;
    float* sV = afs + Tpad * AF_P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int hh = blockIdx.x % heads, b = blockIdx.x / heads;
    const int D = heads * 64;
    const long rs = 3L * D;
    const float* base = qkv + (long)b * Tn * rs + hh * 64;
    af_stage2(sK, base + D, rs, sV, base + 2 * D, rs, Tn, Tpad);
    __syncthreads();
    const float scale2 = scale * 1.4426950408889634f;
    for (int qt = wave; qt < NT; qt += AF_WAVES) {
        const int q0 = qt * 32, qrow = min(q0 + l31, Tn - 1);
        const long orow = ((long)b * Tn + qrow) * D + hh * 64;
        f32x4 qv[8], dov[8];
        float dpart = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            qv[g] = *reinterpret_cast<const f32x4*>(base + (long)qrow * rs + 8 * g + 4 * h);
            dov[g] = *reinterpret_cast<const f32x4*>(d_o + orow + 8 * g + 4 * h);
            const f32x4 ov = *reinterpret_cast<const f32x4*>(o + orow + 8 * g + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) dpart = fmaf(dov[g][c], ov[c], dpart);
        }
        const float Dq = dpart + __shfl_xor(dpart, 32, 64);
        const float lse_q = lse[((long)b * heads + hh) * Tn + qrow];
        f32x16 dq0 = zero16(), dq1 = zero16();
        for (int t = 0; t < NT; ++t) {
            f32x16 s = zero16(), dp = zero16();
            const int ro = (t * 32 + l31) * AF_P + 4 * h;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(sK + ro + 8 * g);
                const f32x4 vf = *reinterpret_cast<const f32x4*>(sV + ro + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s = mfma2(kf[c], qv[g][c], s);                                          // S^T  [key][query]
                    dp = mfma2(vf[c], dov[g][c], dp);                                       // dP^T [key][query]
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = t * 32 + acc_row(r, h) < Tn ? __builtin_amdgcn_exp2f(s[r] * scale2 - lse_q) : 0.f;
                s[r] = p * (dp[r] - Dq);                                                    // dS^T (the factor `scale` at the end)
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* kr = sK + (t * 32 + acc_row(r, h)) * AF_P + l31;
                dq0 = mfma2(kr[0], s[r], dq0);
                dq1 = mfma2(kr[32], s[r], dq1);
            }
        }
        if (q0 + l31 < Tn) {
            float* drow = d_qkv + ((long)b * Tn + q0 + l31) * rs + hh * 64;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4*>(drow + 8 * g + 4 * h) =
                    f32x4{dq0[4 * g] * scale, dq0[4 * g + 1] * scale, dq0[4 * g + 2] * scale, dq0[4 * g + 3] * scale};
                *reinterpret_cast<f32x4*>(drow + 32 + 8 * g + 4 * h) =
                    f32x4{dq1[4 * g] * scale, dq1[4 * g + 1] * scale, dq1[4 * g + 2] * scale, dq1[4 * g + 3] * scale};
            }
        }
    }
}

// dK, dV: a wave owns 32 keys and streams the query tiles of Q and dO from LDS (LSE and D per query beside them):
// S = Q K^T,  dP = dO V^T,  dS = P o (dP - D),  dV^T += dO^T P,  dK^T += Q^T dS.  Writes the k and v thirds of d_qkv.
__global__ __launch_bounds__(AF_THREADS) void attention_f32_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                          const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                          float* __restrict__ d_qkv, int Tn, int heads, float scale, int NT) {
    extern __shared__ __attribute__((aligned(16))) float afs[];
    const int Tpad = 32 * NT;
    float* sQ = afs;
    float* sO = afs + Tpad * AF_P;                 // dO rows
    float* sL = sO + Tpad * AF_P;                  // [Tpad] log-sum-exp (+inf on padding rows: P = 0)
    float* sD = sL + Tpad;                         // [Tpad] D = sum_d dO O
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int hh = blockIdx.x % heads, b = blockIdx.x / heads;
    const int D = heads * 64;
    const long rs = 3L * D;
    const float* base = qkv + (long)b * Tn * rs + hh * 64;
    af_stage2(sQ, base, rs, sO, d_o + (long)b * Tn * D + hh * 64, D, Tn, Tpad);
    __syncthreads();
    for (int i = threadIdx.x; i < Tpad * 16; i += AF_THREADS) {       // 16 lanes per query; Tpad * 16 is a multiple of the block
        const int j = i >> 4, c = i & 15;
        const f32x4 dv = *reinterpret_cast<const f32x4*>(sO + j * AF_P + c * 4);
        const f32x4 ov = *reinterpret_cast<const f32x4*>(o + ((long)b * Tn + min(j, Tn - 1)) * D + hh * 64 + c * 4);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) part = fmaf(dv[e], ov[e], part);
        part += __shfl_xor(part, 1, 64);
        part += __shfl_xor(part, 2, 64);
        part += __shfl_xor(part, 4, 64);
        part += __shfl_xor(part, 8, 64);
        if (c == 0) {
            sD[j] = j < Tn ? part : 0.f;
            sL[j] = j < Tn ? lse[((long)b * heads + hh) * Tn + j] : INFINITY;
        }
    }
    __syncthreads();
    const float scale2 = scale * 1.4426950408889634f;
    for (int kt = wave; kt < NT; kt += AF_WAVES) {
        const int k0 = kt * 32, krow = min(k0 + l31, Tn - 1);
        f32x4 kv[8], vv[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            kv[g] = *reinterpret_cast<const f32x4*>(base + (long)krow * rs + D + 8 * g + 4 * h);
            vv[g] = *reinterpret_cast<const f32x4*>(base + (long)krow * rs + 2 * D + 8 * g + 4 * h);
        }
        f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
        for (int t = 0; t < NT; ++t) {
            f32x16 s = zero16(), dp = zero16();
            const int ro = (t * 32 + l31) * AF_P + 4 * h;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 qf = *reinterpret_cast<const f32x4*>(sQ + ro + 8 * g);
                const f32x4 of = *reinterpret_cast<const f32x4*>(sO + ro + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s = mfma2(qf[c], kv[g][c], s);                                          // S  [query][key]
                    dp = mfma2(of[c], vv[g][c], dp);                                        // dP [query][key]
                }
            }
            f32x16 p;
#pragma unroll
            for (int g = 0; g < 4; ++g) {                                                  // registers 4g .. 4g+3: queries t*32 + 8g + 4h + c
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + t * 32 + 8 * g + 4 * h);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + t * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int r = 4 * g + c;
                    p[r] = __builtin_amdgcn_exp2f(s[r] * scale2 - l4[c]);
                    s[r] = p[r] * (dp[r] - d4[c]);                                          // dS
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro2 = (t * 32 + acc_row(r, h)) * AF_P + l31;
                dv0 = mfma2(sO[ro2], p[r], dv0);
                dv1 = mfma2(sO[ro2 + 32], p[r], dv1);
                dk0 = mfma2(sQ[ro2], s[r], dk0);
                dk1 = mfma2(sQ[ro2 + 32], s[r], dk1);
            }
        }
        if (k0 + l31 < Tn) {
            float* krow_out = d_qkv + ((long)b * Tn + k0 + l31) * rs + D + hh * 64;
            float* vrow_out = krow_out + D;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4*>(krow_out + 8 * g + 4 * h) =
                    f32x4{dk0[4 * g] * scale, dk0[4 * g + 1] * scale, dk0[4 * g + 2] * scale, dk0[4 * g + 3] * scale};
                *reinterpret_cast<f32x4*>(krow_out + 32 + 8 * g + 4 * h) =
                    f32x4{dk1[4 * g] * scale, dk1[4 * g + 1] * scale, dk1[4 * g + 2] * scale, dk1[4 * g + 3] * scale};
                *reinterpret_cast<f32x4*>(vrow_out + 8 * g + 4 * h) = f32x4{dv0[4 * g], dv0[4 * g + 1], dv0[4 * g + 2], dv0[4 * g + 3]};
                *reinterpret_cast<f32x4*>(vrow_out + 32 + 8 * g + 4 * h) = f32x4{dv1[4 * g], dv1[4 * g + 1], dv1[4 * g + 2], dv1[4 * g + 3]};
            }
        }
    }
}

// LayerNorm backward over fp32 rows of D <= 1024 elements (D % 4 == 0): the bf16 kernel of vit_bwd.hip on fp32 storage with a
// whole wave per row, a lane owning the 4-element chunks lane + 64 i (NCH <= 4 of them: the row's registers stay well below the
// spill line).  Each wave walks the rows with a fixed stride and keeps its dgamma / dbeta in registers; one partial row [2][D] per wave.
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_bwd_rows_f32_kernel(const float* __restrict__ x, long xs, const float* __restrict__ gamma,
                                                                     const float* __restrict__ dy, long dys, float eps, const float* __restrict__ add,
                                                                     float* __restrict__ dx, long dxs, float* __restrict__ partial, long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long group = (long)blockIdx.x * 4 + (threadIdx.x >> 6), ngroups = (long)gridDim.x * 4;
    const int nch = D >> 2;
    f32x4 dg[NCH], db[NCH], gm[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        dg[i] = db[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        gm[i] = lane + 64 * i < nch ? *reinterpret_cast<const f32x4*>(gamma + (lane + 64 * i) * 4) : dg[i];
    }
    const float invD = 1.f / (float)D;
    for (long row = group; row < rows; row += ngroups) {
        f32x4 xv[NCH], gv[NCH];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + 64 * i;
            xv[i] = gv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < nch) {
                xv[i] = *reinterpret_cast<const f32x4*>(x + row * xs + c * 4);
                gv[i] = *reinterpret_cast<const f32x4*>(dy + row * dys + c * 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) s += xv[i][e];
        }
        const float mean = wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (lane + 64 * i < nch) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float c = xv[i][e] - mean; xv[i][e] = c; q = fmaf(c, c, q); }
            }
        const float rstd = 1.f / sqrtf(wave_sum(q) * invD + eps);
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {                          // (chunks beyond D hold zeros: no contribution)
                const float xh = xv[i][e] * rstd, d = gv[i][e];
                xv[i][e] = xh;
                dg[i][e] = fmaf(d, xh, dg[i][e]);
                db[i][e] += d;
                const float g = d * gm[i][e];
                gv[i][e] = g;
                sg += g;
                sgx = fmaf(g, xh, sgx);
            }
        }
        sg = wave_sum(sg) * invD;
        sgx = wave_sum(sgx) * invD;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rstd * (gv[i][e] - sg - xv[i][e] * sgx);
                if (add) v += *reinterpret_cast<const f32x4*>(add + row * dxs + c * 4);
                *reinterpret_cast<f32x4*>(dx + row * dxs + c * 4) = v;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            *reinterpret_cast<f32x4*>(partial + (group * 2 + 0) * D + c * 4) = dg[i];
            *reinterpret_cast<f32x4*>(partial + (group * 2 + 1) * D + c * 4) = db[i];
        }
    }
}

// d_y == NULL: y = gelu(u), the erff form of cvcl_gemm's fp32 epilogue (apply_act in gemm.hip, the same expression);
// else y = d_y * gelu'(u), gelu'(u) = 0.5 (1 + erf(u / sqrt 2)) + u exp(-u^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(256) void gelu_f32_kernel(const float* __restrict__ u, const float* __restrict__ d_y, float* __restrict__ y, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(u + i * 4);
        f32x4 r;
        if (d_y) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(d_y + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = a[e];
                const float grad = 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * expf(-0.5f * v * v) * 0.39894228040143267794f;
                r[e] = d[e] * grad;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = 0.5f * a[e] * (1.f + erff(a[e] * 0.70710678118654752440f));
        }
        *reinterpret_cast<f32x4*>(y + i * 4) = r;
    }
}

// backward of cvcl_vit_assemble_tokens on fp32: d_tok[b][p] = dh[b][1 + p];  d_pos[t] = sum over b of dh[b][t], in batch order
__global__ __launch_bounds__(256) void vit_tokens_bwd_f32_kernel(const float* __restrict__ dh, float* __restrict__ d_tok, int B, int T, int D) {
    const long n4 = (long)B * (T - 1) * D / 4, per_img = (long)(T - 1) * D / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long b = i / per_img, r = i - b * per_img;
        *reinterpret_cast<f32x4*>(d_tok + i * 4) = *reinterpret_cast<const f32x4*>(dh + ((long)b * T * D + D) + r * 4);
    }
}
__global__ __launch_bounds__(256) void batch_sum_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int B, long n) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n / 4; j += (long)gridDim.x * blockDim.x) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int b0 = 0; b0 < B; b0 += 8) {                  // eight rows' loads in flight per wait, added in batch order
            f32x4 a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const f32x4*>(x + (long)min(b0 + u, B - 1) * n + j * 4);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (b0 + u < B) acc += a[u];
        }
        *reinterpret_cast<f32x4*>(out + j * 4) = acc;
    }
}

// ---- dW = A^T B, colsum(A) on v_mfma_f32_32x32x2_f32 ------------------------------------------------------------------------------
// A = dY [M][lda], B = X [M][ldb], both row-major as the forward left them.  The contraction runs over the rows m, which is the
// MFMA's k: a step takes rows (m, m+1), lane half h supplies row m + h, and its 32 lanes read 32 consecutive floats of that row --
// A[m+h][n0 + l31] and B[m+h][k0 + l31] are exactly the A and B operand maps, so the operands go from global memory (L2) straight
// into the MFMA with no LDS.  Workgroup = 4 waves on a 128 (n) x 128 (k) tile, a wave 2 x 2 tiles of 32 x 32; blockIdx.z = one of
// S chunks of the rows.  Each workgroup writes its partial tile to the workspace [S][N][K]; a second kernel adds the S partials in
// chunk order (deterministic).  The A values a lane loads are also summed (colsum partial [S][N], written by the k-tile-0 waves).
constexpr int TF_T = 128;
constexpr int TF_UN = 8;                // row pairs in flight per lane

struct TfPlan { int S; long chunk; int tn, tk; };
TfPlan tf_plan(long M, int N, int K) {
    TfPlan p;
    p.tn = cvcl_div_up(N, TF_T);
    p.tk = cvcl_div_up(K, TF_T);
    const long tiles = (long)p.tn * p.tk;
    long S = (2048 + tiles - 1) / tiles;                     // ~8 workgroups of 4 waves per CU
    const long smax = (M + 255) / 256;                       // at least 256 rows per chunk
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    p.chunk = ((M + S - 1) / S + 2 * TF_UN - 1) / (2 * TF_UN) * (2 * TF_UN);
    p.S = (int)((M + p.chunk - 1) / p.chunk);
    return p;
}

__global__ __launch_bounds__(256) void gemm_tn_f32_partial_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                                                  long M, int N, int K, long chunk, float* __restrict__ part,
                                                                  float* __restrict__ cpart) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * TF_T + (wave & 1) * 64, k0 = blockIdx.y * TF_T + (wave >> 1) * 64;
    const long m_begin = (long)blockIdx.z * chunk, m_end = min(M, m_begin + chunk);
    const int na0 = min(n0 + l31, N - 1), na1 = min(n0 + 32 + l31, N - 1);
    const int kb0 = min(k0 + l31, K - 1), kb1 = min(k0 + 32 + l31, K - 1);
    f32x16 c00 = zero16(), c01 = zero16(), c10 = zero16(), c11 = zero16();
    float cs0 = 0.f, cs1 = 0.f;
    for (long mm = m_begin; mm < m_end; mm += 2 * TF_UN) {
        float a0[TF_UN], a1[TF_UN], b0[TF_UN], b1[TF_UN];
#pragma unroll
        for (int u = 0; u < TF_UN; ++u) {
            const long row = mm + 2 * u + h;
            const long rr = row < m_end ? row : m_begin;
            a0[u] = A[rr * lda + na0];
            a1[u] = A[rr * lda + na1];
            b0[u] = Bm[rr * ldb + kb0];
            b1[u] = Bm[rr * ldb + kb1];
        }
#pragma unroll
        for (int u = 0; u < TF_UN; ++u) {
            if (mm + 2 * u + h >= m_end) a0[u] = a1[u] = b0[u] = b1[u] = 0.f;
            c00 = mfma2(a0[u], b0[u], c00);
            c01 = mfma2(a0[u], b1[u], c01);
            c10 = mfma2(a1[u], b0[u], c10);
            c11 = mfma2(a1[u], b1[u], c11);
            cs0 += a0[u];
            cs1 += a1[u];
        }
    }
    float* P = part + (long)blockIdx.z * N * K;
    const int ka = k0 + l31, kb = k0 + 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int na = n0 + acc_row(r, h), nb = n0 + 32 + acc_row(r, h);
        if (na < N) {
            if (ka < K) P[(long)na * K + ka] = c00[r];
            if (kb < K) P[(long)na * K + kb] = c01[r];
        }
        if (nb < N) {
            if (ka < K) P[(long)nb * K + ka] = c10[r];
            if (kb < K) P[(long)nb * K + kb] = c11[r];
        }
    }
    cs0 += __shfl_xor(cs0, 32, 64);
    cs1 += __shfl_xor(cs1, 32, 64);
    if (blockIdx.y == 0 && (wave >> 1) == 0 && h == 0) {
        if (n0 + l31 < N) cpart[(long)blockIdx.z * N + n0 + l31] = cs0;
        if (n0 + 32 + l31 < N) cpart[(long)blockIdx.z * N + n0 + 32 + l31] = cs1;
    }
}

__global__ __launch_bounds__(256) void gemm_tn_f32_reduce_kernel(const float* __restrict__ part, const float* __restrict__ cpart, int S, int N,
                                                                 int K, int k_keep, float* __restrict__ C, float* __restrict__ colsum) {
    const long total = (long)N * k_keep;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total + N; i += (long)gridDim.x * blockDim.x) {
        float acc = 0.f;
        if (i < total) {
            const long n = i / k_keep, k = i - n * k_keep;
            for (int s = 0; s < S; ++s) acc += part[((long)s * N + n) * K + k];
            C[i] = acc;
        } else {
            const long n = i - total;
            for (int s = 0; s < S; ++s) acc += cpart[(long)s * N + n];
            colsum[n] = acc;
        }
    }
}

}  // namespace

// qkv [B][T][3][heads][64] fp32 -> out [B][T][heads*64] fp32, lse [B][heads][T] fp32 (log2 units, as cvcl_attention_train).
// head_dim 64, 32 < T <= 288; all pointers 16-byte aligned.
extern "C" int cvcl_attention_train_f32(const float* qkv, float* out, float* lse, int B, int T, int heads, int head_dim, float scale,
                                        void* stream) {
    CVCL_CHECK_ARG(qkv && out && lse && B > 0 && heads > 0, "cvcl_attention_train_f32: bad args");
    CVCL_CHECK_ARG(head_dim == 64 && T > 32 && T <= AF_TPAD_MAX, "cvcl_attention_train_f32: needs head_dim 64 and 32 < T <= %d (got hd %d, T %d)",
                   AF_TPAD_MAX, head_dim, T);
    CVCL_CHECK_ARG(cvcl_aligned16(qkv) && cvcl_aligned16(out), "cvcl_attention_train_f32: qkv / out must be 16-byte aligned");
    static CvclLdsAttr attr;
    if (const int rc = cvcl_raise_lds_limit(attr, (const void*)attention_f32_fwd_kernel, 160 * 1024, "cvcl_attention_train_f32")) return rc;
    attr.mark();
    const int nt = (T + 31) / 32;
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    hipLaunchKernelGGL(attention_f32_fwd_kernel, dim3(B * heads), dim3(AF_THREADS), (size_t)nt * 32 * AF_P * 4 * 2, (hipStream_t)stream, qkv,
                       out, lse, T, heads, scale, nt);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// qkv, o, d_o, lse as cvcl_attention_bwd but fp32 -> d_qkv [B][T][3][heads][64] fp32, fully written.  head_dim 64, 32 < T <= 288.
extern "C" int cvcl_attention_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse, float* d_qkv, int B, int T,
                                      int heads, int head_dim, float scale, void* stream) {
    CVCL_CHECK_ARG(qkv && o && d_o && lse && d_qkv && B > 0 && heads > 0, "cvcl_attention_bwd_f32: bad args");
    CVCL_CHECK_ARG(head_dim == 64 && T > 32 && T <= AF_TPAD_MAX, "cvcl_attention_bwd_f32: needs head_dim 64 and 32 < T <= %d (got hd %d, T %d)",
                   AF_TPAD_MAX, head_dim, T);
    CVCL_CHECK_ARG(cvcl_aligned16(qkv) && cvcl_aligned16(o) && cvcl_aligned16(d_o) && cvcl_aligned16(d_qkv), "cvcl_attention_bwd_f32: operands must be 16-byte aligned");
    static CvclLdsAttr attr;
    if (const int rc = cvcl_raise_lds_limit(attr, (const void*)attention_f32_bwd_dq_kernel, 160 * 1024, "cvcl_attention_bwd_f32")) return rc;
    if (const int rc = cvcl_raise_lds_limit(attr, (const void*)attention_f32_bwd_dkv_kernel, 160 * 1024, "cvcl_attention_bwd_f32")) return rc;
    attr.mark();
    const int nt = (T + 31) / 32, Tpad = nt * 32;
    hipStream_t s = (hipStream_t)stream;
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    hipLaunchKernelGGL(attention_f32_bwd_dq_kernel, dim3(B * heads), dim3(AF_THREADS), (size_t)Tpad * AF_P * 4 * 2, s, qkv, o, d_o, lse, d_qkv,
                       T, heads, scale, nt);
    hipLaunchKernelGGL(attention_f32_bwd_dkv_kernel, dim3(B * heads), dim3(AF_THREADS), (size_t)Tpad * AF_P * 4 * 2 + (size_t)Tpad * 8, s, qkv,
                       o, d_o, lse, d_qkv, T, heads, scale, nt);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// fp32 rows: x, dy, add (nullable, dx's layout), dx; partial [cvcl_layernorm_bwd_rows_partials(rows)][2][D].  D % 4 == 0, D <= 1024.
extern "C" int cvcl_layernorm_bwd_rows_f32(const float* x, long x_row_stride, const float* gamma, const float* dy, long dy_row_stride, float eps,
                                           const float* add, float* dx, long dx_row_stride, float* partial, long rows, int D, void* stream) {
    CVCL_CHECK_ARG(x && gamma && dy && dx && partial && rows > 0 && D > 0, "cvcl_layernorm_bwd_rows_f32: bad args");
    CVCL_CHECK_ARG(D % 4 == 0 && D <= 1024 && x_row_stride % 4 == 0 && dy_row_stride % 4 == 0 && dx_row_stride % 4 == 0 && cvcl_aligned16(x) &&
                       cvcl_aligned16(dy) && cvcl_aligned16(dx) && cvcl_aligned16(gamma) && cvcl_aligned16(add) && cvcl_aligned16(partial),
                   "cvcl_layernorm_bwd_rows_f32: needs D %% 4 == 0, D <= 1024 and 16-byte aligned rows (D %d)", D);
    const int wgs = cvcl_layernorm_bwd_rows_partials(rows) / 4;          // one partial row per wave: exactly that many rows written
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    hipStream_t s = (hipStream_t)stream;
#define CVCL_LNB(NCH_) hipLaunchKernelGGL(layernorm_bwd_rows_f32_kernel<NCH_>, dim3(wgs), dim3(256), 0, s, x, x_row_stride, gamma, dy, \
                                          dy_row_stride, eps, add, dx, dx_row_stride, partial, rows, D)
    if (D <= 256) CVCL_LNB(1);
    else if (D <= 512) CVCL_LNB(2);
    else if (D <= 768) CVCL_LNB(3);
    else CVCL_LNB(4);
#undef CVCL_LNB
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_gelu_f32(const float* u, const float* d_y, float* y, long n, void* stream) {
    CVCL_CHECK_ARG(u && y && n > 0 && n % 4 == 0 && cvcl_aligned16(u) && cvcl_aligned16(d_y) && cvcl_aligned16(y), "cvcl_gelu_f32: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(gelu_f32_kernel, dim3(cvcl_grid(n / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, u, d_y, y, n / 4);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_vit_tokens_bwd_f32(const float* dh, float* d_tok, float* d_pos, int B, int T, int D, void* stream) {
    CVCL_CHECK_ARG(dh && d_tok && d_pos && B > 0 && T > 1 && D > 0 && D % 4 == 0 && cvcl_aligned16(dh) && cvcl_aligned16(d_tok) && cvcl_aligned16(d_pos),
                   "cvcl_vit_tokens_bwd_f32: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(vit_tokens_bwd_f32_kernel, dim3(cvcl_grid((long)B * (T - 1) * D / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, dh, d_tok,
                       B, T, D);
    hipLaunchKernelGGL(batch_sum_f32_kernel, dim3(cvcl_grid((long)T * D / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, dh, d_pos, B, (long)T * D);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" size_t cvcl_gemm_tn_colsum_f32_workspace_bytes(long M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const TfPlan p = tf_plan(M, N, K);
    return ((size_t)p.S * N * K + (size_t)p.S * N) * sizeof(float);
}

// fp32 A [M][lda >= N], B [M][ldb >= K] -> C [N][k_keep] = (A^T B)[:, :k_keep], colsum [N] = column sums of A
extern "C" int cvcl_gemm_tn_colsum_f32(const float* A, int lda, const float* B, int ldb, long M, int N, int K, float* C, int k_keep,
                                       float* colsum, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(A && B && C && colsum && workspace && M > 0 && N > 0 && K > 0 && lda >= N && ldb >= K && k_keep > 0 && k_keep <= K,
                   "cvcl_gemm_tn_colsum_f32: bad args");
    if (workspace_bytes < cvcl_gemm_tn_colsum_f32_workspace_bytes(M, N, K)) {
        cvcl_set_error("cvcl_gemm_tn_colsum_f32: workspace too small");
        return CVCL_EWORKSPACE;
    }
    const TfPlan p = tf_plan(M, N, K);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    float* cpart = part + (size_t)p.S * N * K;
    CvclProfScope prof(stream, CVCL_K_WGRAD);
    hipLaunchKernelGGL(gemm_tn_f32_partial_kernel, dim3(p.tn, p.tk, p.S), dim3(256), 0, s, A, lda, B, ldb, M, N, K, p.chunk, part, cpart);
    hipLaunchKernelGGL(gemm_tn_f32_reduce_kernel, dim3(cvcl_grid((long)N * k_keep + N, 256, 8192)), dim3(256), 0, s, (const float*)part,
                       (const float*)cpart, p.S, N, K, k_keep, C, colsum);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
