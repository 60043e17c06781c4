// Text-encoder kernels that are not a GEMM and not the LSTM (csrc/lstm.hip): the embedding(+pos) gather, sequence pooling, CBOW,
// dropout, and the training side of the one-layer text transformer (reference multimodal/multimodal.py:496-573 run under Lightning's
// .train()): LayerNorm / ReLU backward and the small masked attention.  All fp32, deterministic (no atomics).
#include "cvcl_common.h"

namespace {

// x[b][l][:] = table[tok[b][l]] (+ pos[l])                       (multimodal.py:496, 561-563)
__global__ __launch_bounds__(256) void embed_gather_pos_kernel(const float* __restrict__ table, const int64_t* __restrict__ tok,
                                                               const float* __restrict__ pos, float* __restrict__ x, int B,
                                                               int L, int E, int V) {
    const long total = (long)B * L * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const long r = i / E;
        const int l = (int)(r % L);
        const int64_t t = tok[r];
        float v = (t >= 0 && t < V) ? table[t * E + e] : NAN;
        if (pos) v += pos[(long)l * E + e];
        x[i] = v;
    }
}

// ret[b][:] = sum_l x[b][l][:] / len[b]   (all L positions, pads included: multimodal.py:573, Appendix C.1)
__global__ __launch_bounds__(256) void seq_sum_div_kernel(const float* __restrict__ x, const int64_t* __restrict__ len,
                                                          float* __restrict__ ret, int B, int L, int E) {
    const long total = (long)B * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const long b = i / E;
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc += x[(b * L + l) * E + e];
        ret[i] = acc / (float)len[b];
    }
}

// dx[b,l,:] = d_ret[b,:] / len[b] for every l (backward of seq_sum_div: pads included, as in the forward)
__global__ __launch_bounds__(256) void seq_sum_div_bwd_kernel(const float* __restrict__ d_ret, const int64_t* __restrict__ len,
                                                              float* __restrict__ dx, int B, int L, int E) {
    const long total = (long)B * L * E;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const long b = i / ((long)L * E);
        dx[i] = d_ret[b * E + e] / (float)len[b];
    }
}

// continuous bag of words: y[b][j] = (sum_{|k-j| <= c, k != j, 0 <= k < L} x[b][k]) / (2c); symmetric -> its own backward
__global__ __launch_bounds__(256) void cbow_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int L, int E, int c) {
    const long total = (long)B * L * E;
    const float inv = 1.f / (float)(2 * c);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const long r = i / E;
        const int j = (int)(r % L);
        const long b = r / L;
        float acc = 0.f;
        for (int k = max(j - c, 0); k <= min(j + c, L - 1); ++k)
            if (k != j) acc += x[(b * L + k) * E + e];
        y[i] = acc * inv;
    }
}

// counter-based hash RNG (one draw per element): keep iff u >= p.  Same (seed, index) -> same mask in fwd and bwd.
__device__ inline float hash_uniform(unsigned long long seed, unsigned long long idx) {
    unsigned long long z = seed + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);          // 24 random bits -> [0, 1)
}

// y = x * keep / (1 - p); the same kernel is the backward (dx = dy * keep / (1 - p)).
// period > 0: the mask index is (i / (period * inner)) * inner + i % inner, i.e. shared along one dimension
// (LockedDropout, multimodal.py:46-53: mask shape [B,1,E] shared over time).
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                      float* __restrict__ y, long n, float p, unsigned long long seed,
                                                      long period, long inner) {
    const float scale = 1.f / (1.f - p);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long mi = period > 0 ? (i / (period * inner)) * inner + (i % inner) : i;
        float v = (p <= 0.f || hash_uniform(seed, (unsigned long long)mi) >= p) ? x[i] * scale : 0.f;
        if (res) v += res[i];
        y[i] = v;
    }
}

// LayerNorm backward, one wave per row: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma.
// Per-row partial products for dgamma / dbeta are written as dy*xhat and dy (reduced by cvcl_colsum_f32).
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, float eps, float* __restrict__ dx,
                                                            float* __restrict__ dyxhat, long rows, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + row * D;
    const float* gr = dy + row * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += xr[d];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) { const float c = xr[d] - mean; q = fmaf(c, c, q); }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
    float sg = 0.f, sgx = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float xh = (xr[d] - mean) * rstd, g = gr[d] * gamma[d];
        sg += g;
        sgx = fmaf(g, xh, sgx);
    }
    sg = wave_sum(sg) / (float)D;
    sgx = wave_sum(sgx) / (float)D;
    for (int d = lane; d < D; d += 64) {
        const float xh = (xr[d] - mean) * rstd, g = gr[d] * gamma[d];
        dx[row * D + d] = rstd * (g - sg - xh * sgx);
        dyxhat[row * D + d] = gr[d] * xh;
    }
}

// dx = dy where y > 0 (ReLU backward from the saved output)
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                       float* __restrict__ dx, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// Small-sequence attention forward+backward with key padding mask and probability dropout (training).
// One workgroup (64 threads = 1 wave) per (b, head); T <= 32, hd <= 128.  P is recomputed in the backward.
//   S = q k^T * scale (+mask) ; P = softmax(S) ; Pd = dropout(P) ; O = Pd v
//   dPd = dO v^T ; dP = dropout'(dPd) ; dS = P * (dP - sum_j dP P) ; dq = dS k * scale ; dk = dS^T q * scale ; dv = Pd^T dO
constexpr int SA_T = 32;
__global__ __launch_bounds__(64) void attn_small_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ key_tok,
                                                        const float* __restrict__ d_out, float* __restrict__ out,
                                                        float* __restrict__ d_qkv, int B, int T, int heads, int hd,
                                                        float scale, float p, unsigned long long seed) {
    __shared__ float sP[SA_T][SA_T + 1], sPd[SA_T][SA_T + 1], sdS[SA_T][SA_T + 1];
    const int lane = threadIdx.x;
    const int hh = blockIdx.x % heads, b = blockIdx.x / heads;
    const int D = heads * hd;
    const float* base = qkv + (long)b * T * 3 * D;
    const float keep_scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
    // scores: lane handles pairs (i, j) = idx / T, idx % T
    for (int idx = lane; idx < T * T; idx += 64) {
        const int i = idx / T, j = idx - i * T;
        const float* qp = base + (long)i * 3 * D + hh * hd;
        const float* kp = base + (long)j * 3 * D + D + hh * hd;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(qp[d], kp[d], s);
        s *= scale;
        if (key_tok && key_tok[(long)b * T + j] == 0) s = -INFINITY;
        sP[i][j] = s;
    }
    __syncthreads();
    if (lane < T) {                                       // row softmax + dropout mask
        const int i = lane;
        float mx = -INFINITY;
        for (int j = 0; j < T; ++j) mx = fmaxf(mx, sP[i][j]);
        float sum = 0.f;
        for (int j = 0; j < T; ++j) { const float e = expf(sP[i][j] - mx); sP[i][j] = e; sum += e; }
        for (int j = 0; j < T; ++j) {
            const float pr = sP[i][j] / sum;
            sP[i][j] = pr;
            float keep = 1.f;
            if (p > 0.f) keep = hash_uniform(seed, (((unsigned long long)b * heads + hh) * T + i) * T + j) >= p ? keep_scale : 0.f;
            sPd[i][j] = pr * keep;
        }
    }
    __syncthreads();
    if (out) {
        for (int idx = lane; idx < T * hd; idx += 64) {
            const int i = idx / hd, d = idx - i * hd;
            float acc = 0.f;
            for (int j = 0; j < T; ++j) acc = fmaf(sPd[i][j], base[(long)j * 3 * D + 2 * D + hh * hd + d], acc);
            out[((long)b * T + i) * D + hh * hd + d] = acc;
        }
    }
    if (!d_qkv) return;
    const float* dO = d_out + (long)b * T * D;
    float* dbase = d_qkv + (long)b * T * 3 * D;
    // dPd[i][j] = dO[i] . v[j]; dP = dPd * keep
    for (int idx = lane; idx < T * T; idx += 64) {
        const int i = idx / T, j = idx - i * T;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(dO[(long)i * D + hh * hd + d], base[(long)j * 3 * D + 2 * D + hh * hd + d], s);
        float keep = 1.f;
        if (p > 0.f) keep = hash_uniform(seed, (((unsigned long long)b * heads + hh) * T + i) * T + j) >= p ? keep_scale : 0.f;
        sdS[i][j] = s * keep;
    }
    __syncthreads();
    if (lane < T) {
        const int i = lane;
        float dot = 0.f;
        for (int j = 0; j < T; ++j) dot = fmaf(sdS[i][j], sP[i][j], dot);
        for (int j = 0; j < T; ++j) sdS[i][j] = sP[i][j] * (sdS[i][j] - dot);
    }
    __syncthreads();
    for (int idx = lane; idx < T * hd; idx += 64) {
        const int i = idx / hd, d = idx - i * hd;
        float dq = 0.f, dk = 0.f, dv = 0.f;
        for (int j = 0; j < T; ++j) {
            dq = fmaf(sdS[i][j], base[(long)j * 3 * D + D + hh * hd + d], dq);       // dS[i][j] * k[j]
            dk = fmaf(sdS[j][i], base[(long)j * 3 * D + hh * hd + d], dk);           // dS[j][i] * q[j]
            dv = fmaf(sPd[j][i], dO[(long)j * D + hh * hd + d], dv);                 // Pd[j][i] * dO[j]
        }
        dbase[(long)i * 3 * D + hh * hd + d] = dq * scale;
        dbase[(long)i * 3 * D + D + hh * hd + d] = dk * scale;
        dbase[(long)i * 3 * D + 2 * D + hh * hd + d] = dv;
    }
}

// y = alpha * (a + b)   (b may be NULL): mean of the two LSTM directions and its backward
__global__ __launch_bounds__(256) void scale_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float alpha,
                                                        float* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = alpha * (a[i] + (b ? b[i] : 0.f));
}

// CLIP's text pooling: out[b][:] = LayerNorm(x[b][argmax_l tok[b][l]][:]) -- the end-of-text id is the largest id, the first maximum
// wins (torch.argmax).  One wave per sequence; the LayerNorm is the arithmetic of cvcl_layernorm's scalar kernel (vit.hip).
__global__ __launch_bounds__(256) void clip_text_pool_kernel(const float* __restrict__ x, const int64_t* __restrict__ tok,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             float* __restrict__ out, int B, int L, int W) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int64_t* tb = tok + (long)b * L;
    long long best = tb[0];
    int at = 0;
    for (int l = lane; l < L; l += 64) {                     // ascending l per lane: a strict > keeps the lane's first maximum
        const long long t = tb[l];
        if (t > best) { best = t; at = l; }
    }
    for (int o = 32; o > 0; o >>= 1) {                       // (id desc, position asc): the same winner in every lane
        const long long t = __shfl_xor(best, o, 64);
        const int l = __shfl_xor(at, o, 64);
        if (t > best || (t == best && l < at)) { best = t; at = l; }
    }
    const float* xr = x + ((long)b * L + at) * W;
    float s = 0.f;
    for (int d = lane; d < W; d += 64) s += xr[d];
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
    for (int d = lane; d < W; d += 64) {
        const float c = xr[d] - mean;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)W + eps);
    for (int d = lane; d < W; d += 64) out[(long)b * W + d] = (xr[d] - mean) * rstd * gamma[d] + beta[d];
}

}  // namespace

// ================================================================================================
extern "C" int cvcl_embed_gather_pos(const float* table, const int64_t* tok, const float* pos, float* x, int B, int L, int E,
                                     int V, void* stream) {
    CVCL_CHECK_ARG(table && tok && x && B > 0 && L > 0 && E > 0 && V > 0, "cvcl_embed_gather_pos: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(embed_gather_pos_kernel, dim3(cvcl_grid((long)B * L * E, 256, 8192)), dim3(256), 0, (hipStream_t)stream, table, tok,
                       pos, x, B, L, E, V);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_seq_sum_div(const float* x, const int64_t* len, float* ret, int B, int L, int E, void* stream) {
    CVCL_CHECK_ARG(x && len && ret && B > 0 && L > 0 && E > 0, "cvcl_seq_sum_div: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(seq_sum_div_kernel, dim3(cvcl_grid((long)B * E, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, len, ret, B, L, E);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_seq_sum_div_bwd(const float* d_ret, const int64_t* len, float* dx, int B, int L, int E, void* stream) {
    CVCL_CHECK_ARG(d_ret && len && dx && B > 0 && L > 0 && E > 0, "cvcl_seq_sum_div_bwd: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(seq_sum_div_bwd_kernel, dim3(cvcl_grid((long)B * L * E, 256, 8192)), dim3(256), 0, (hipStream_t)stream, d_ret, len, dx,
                       B, L, E);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_cbow(const float* x, float* y, int B, int L, int E, int crange, void* stream) {
    CVCL_CHECK_ARG(x && y && x != y && B > 0 && L > 0 && E > 0 && crange > 0, "cvcl_cbow: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(cbow_kernel, dim3(cvcl_grid((long)B * L * E, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, y, B, L, E, crange);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_dropout(const float* x, const float* residual, float* y, long n, float p, unsigned long long seed,
                            long shared_period, long inner, void* stream) {
    CVCL_CHECK_ARG(x && y && n > 0 && p >= 0.f && p < 1.f, "cvcl_dropout: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(dropout_kernel, dim3(cvcl_grid(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, residual, y, n, p, seed,
                       shared_period, inner > 0 ? inner : 1);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, float* dx, float* dy_xhat,
                                  long rows, int D, void* stream) {
    CVCL_CHECK_ARG(x && gamma && dy && dx && dy_xhat && rows > 0 && D > 0, "cvcl_layernorm_bwd: bad args");
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(cvcl_div_up(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, dy, eps, dx,
                       dy_xhat, rows, D);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_relu_bwd(const float* y, const float* dy, float* dx, long n, void* stream) {
    CVCL_CHECK_ARG(y && dy && dx && n > 0, "cvcl_relu_bwd: bad args");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(cvcl_grid(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, y, dy, dx, n);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_attention_small(const float* qkv, const int64_t* key_tok, const float* d_out, float* out, float* d_qkv,
                                    int B, int T, int heads, int head_dim, float scale, float dropout_p,
                                    unsigned long long seed, void* stream) {
    CVCL_CHECK_ARG(qkv && (out || d_qkv) && B > 0 && T > 0 && T <= SA_T && heads > 0 && head_dim > 0,
                   "cvcl_attention_small: bad args (T <= %d)", SA_T);
    CVCL_CHECK_ARG(!d_qkv || d_out, "cvcl_attention_small: d_out needed for the backward");
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    hipLaunchKernelGGL(attn_small_kernel, dim3(B * heads), dim3(64), 0, (hipStream_t)stream, qkv, key_tok, d_out, out, d_qkv, B, T,
                       heads, head_dim, scale, dropout_p, seed);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_scale_add_f32(const float* a, const float* b, float alpha, float* y, long n, void* stream) {
    CVCL_CHECK_ARG(a && y && n > 0, "cvcl_scale_add_f32: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(scale_add_kernel, dim3(cvcl_grid(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, a, b, alpha, y, n);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// the end-of-text pooling + ln_final of CLIP's encode_text (the reference's --clip_eval baseline, eval.py:205-207, 224-226)
extern "C" int cvcl_clip_text_pool(const float* x, const int64_t* tok, const float* gamma, const float* beta, float eps, float* out, int B,
                                   int L, int W, void* stream) {
    CVCL_CHECK_ARG(x && tok && gamma && beta && out && B > 0 && L > 0 && W > 0, "cvcl_clip_text_pool: bad args");
    CvclProfScope prof(stream, CVCL_K_LAYERNORM);
    hipLaunchKernelGGL(clip_text_pool_kernel, dim3(cvcl_div_up(B, 4)), dim3(256), 0, (hipStream_t)stream, x, tok, gamma, beta, eps, out, B, L,
                       W);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
