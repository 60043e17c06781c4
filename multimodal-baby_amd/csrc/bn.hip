// BatchNorm and the other elementwise passes of the ResNeXt-50 trunk for gfx950 (reference: the nn.BatchNorm2d, ReLU, MaxPool2d and
// AdaptiveAvgPool2d modules of torchvision.models.resnext50_32x4d, reached at multimodal/multimodal.py:101 through
// VisionEncoder.forward; the grouped pass: eval_linear_decoding.py:53-57, 89-91, which never calls .eval()).
//
// Activations are NHWC.  "raw" tensors are convolution outputs *before* BatchNorm: every convolution kernel also emits per-channel
// sum / sum-of-squares partial rows of what it stored (col_stats does it for the fp32 parity kernels), bn_finalize turns them into a
// per-channel (scale, shift) and updates the running statistics, and the *consumer* of the raw tensor applies scale/shift(+ReLU)
// while loading.  A normalised tensor is materialised only where the network needs it twice (block outputs, max-pool output):
//
//   bn_finalize / bn_eval_affine[_all] / bn_apply_moments : statistics -> affine, running statistics (one launch over all 53 layers
//                                                           for eval mode and for the deferred update)
//   bn_relu_maxpool, bn_relu_apply, bn_add_relu, avgpool  : the passes that materialise a normalised tensor
//   bn_group_*                                            : the same for a batch of T groups, each normalised on its own statistics
// The launchers of the trunk walk (csrc/resnext.hip) are declared in cvcl_common.h.
#include <algorithm>

#include "cvcl_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// BatchNorm bookkeeping
// ------------------------------------------------------------------------------------------------
// stats [rows][2][C] partial sums -> scale = gamma / sqrt(var + eps), shift = beta - mean * scale;
// running_mean/var EMA with the unbiased variance (nn.BatchNorm2d train mode), num_batches_tracked += 1.
// the running-statistics update r <- (1 - m) r + m x: one spelling, shared by the in-place and the deferred form (identical bits)
// (bn_ema lives in cvcl_common.h: shared with the finalize-on-load consumers)

// moments != NULL: the batch mean / unbiased variance are written there ([2][C]) and the running statistics are left alone --
// `bn_apply_moments_kernel` applies them later (cvcl_resnext50_fwd_deferred_stats: passes pipelined on two streams).
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ stats, int rows, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           int64_t* __restrict__ nbt, float momentum, float eps,
                                                           float* __restrict__ scale, float* __restrict__ shift, int C,
                                                           float* __restrict__ moments, int moments_ld,
                                                           const float* __restrict__ centre) {
    // 16 channels x 64 row slices per workgroup (short dependent-load chains: the early layers have 512 partial rows and
    // only 64-256 channels); slices combined in a fixed order (deterministic)
    constexpr int NS = 64, NC = 16;
    __shared__ double ps[NS][NC], pq[NS][NC];
    const int c = threadIdx.x & (NC - 1), sl = threadIdx.x / NC, ch = blockIdx.x * NC + c;
    double s = 0.0, q = 0.0;
    if (ch < C) {
        // eight rows' loads are issued before the first is added (same summation order): one wait per eight rows instead of a
        // dependent L2 round trip per row -- the kernel is nothing but latency
        constexpr int UN = 8;
        for (int r0 = sl; r0 < rows; r0 += NS * UN) {
            float a[UN], b[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int r = min(r0 + NS * u, rows - 1);                       // clamped: always a valid address, no branch
                a[u] = stats[((long)r * 2 + 0) * C + ch];
                b[u] = stats[((long)r * 2 + 1) * C + ch];
            }
#pragma unroll
            for (int u = 0; u < UN; ++u)
                if (r0 + NS * u < rows) { s += (double)a[u]; q += (double)b[u]; }
        }
    }
    ps[sl][c] = s;
    pq[sl][c] = q;
    __syncthreads();
    if (sl == 0 && ch < C) {
        s = 0.0; q = 0.0;
        for (int i = 0; i < NS; ++i) { s += ps[i][c]; q += pq[i][c]; }
        // the statistics are those of the STORED tensor y - c (centred storage): (scale, shift) apply to it as it lies in memory;
        // the mean of y itself, for the running statistics, is mean + c
        const double mean = s / count;
        double var = q / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float sc = gamma[ch] / sqrtf((float)var + eps);
        scale[ch] = sc;
        shift[ch] = beta[ch] - (float)mean * sc;
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        const float true_mean = centre ? (float)(mean + (double)centre[ch]) : (float)mean;
        if (moments) {
            moments[ch] = true_mean;
            moments[moments_ld + ch] = (float)unbiased;
        } else if (running_mean) {
            running_mean[ch] = bn_ema(running_mean[ch], true_mean, momentum);
            running_var[ch] = bn_ema(running_var[ch], (float)unbiased, momentum);
        }
    }
    if (!moments && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}

// ---- finalize-on-load (round 6; BnSrc / bn_slice_affine in cvcl_common.h) ---------------------------------------------------------------
// bn_finalize is a 5 us kernel of dependent L2 round trips between a convolution and the consumer of its output: 45 launches per
// pass, each with two kernel boundaries on the trunk's dependent chain.  Where the consumer's workgroups normalise a FIXED set of
// channels -- the grouped 3x3's 64-channel slabs (BN1 of all 16 Bottlenecks), the Gram launch's K <= 256 operand columns (BN2 of
// layers 1-2) -- the producing convolution ACCUMULATES its partial sums instead of writing partial rows (int64 fixed point, one row
// per XCD: order-independent = deterministic) and the consumer forms its channels' (scale, shift) in its prologue: one round trip of
// 16 independent loads per channel, no launch; the workgroup with ``publish`` set also leaves the batch moments / running statistics
// (and the affine, for later readers) behind.  61 -> 38 launches of the bn_finalize class per pass; one pass in flight 5.66 -> 5.46 ms
// per C2 step, two passes in flight unchanged (the other pass already ran in those gaps) -- profiles/r06_fol_ab.txt, which also holds
// what was measured and dropped: partial ROWS reduced redundantly in every consumer workgroup (bit-identical to bn_finalize, but 3-8 us
// of dependent loads and an ordered fp64 chain inside every consumer: no gain), and channel-sliced 1024-thread forms of the
// elementwise passes of layers 3-4 finalizing BN2 / BN3 on load (18 launches left, but 2-3 us more per pass than the launch saved).

// deferred running-statistics update of the whole trunk: all 53 layers in one launch, from the moments a pass left behind
// (ApplyMomentsAll: cvcl_common.h)
__global__ __launch_bounds__(256) void bn_apply_moments_kernel(ApplyMomentsAll t, const float* __restrict__ moments, float momentum) {
    const int l = blockIdx.x;
    const float* m = moments + (size_t)l * kAffStride;
    for (int ch = threadIdx.x; ch < t.C[l]; ch += 256) {
        t.rm[l][ch] = bn_ema(t.rm[l][ch], m[ch], momentum);
        t.rv[l][ch] = bn_ema(t.rv[l][ch], m[kMaxC + ch], momentum);
    }
    if (threadIdx.x == 0 && t.nbt[l]) *t.nbt[l] += 1;
}

__global__ void bn_eval_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                      float* __restrict__ scale, float* __restrict__ shift, const float* __restrict__ centre, int C) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < C) {
        const float sc = gamma[ch] / sqrtf(rv[ch] + eps);
        scale[ch] = sc;
        shift[ch] = beta[ch] - (centre ? rm[ch] - centre[ch] : rm[ch]) * sc;      // affine of the tensor stored as y - c
    }
}

// eval mode of the whole trunk: all 53 (scale, shift) pairs from the running statistics in ONE launch (the layer table
// travels by value in the kernel argument block: EvalAffineAll, cvcl_common.h), instead of 53 dependent 4-us launches on the
// latency path
// centres: the storage centres the pass will use ([53][2048], "Centred storage" in cvcl_hip.h); NULL with centres_out: the
// running means themselves, which this kernel then writes to centres_out for the convolutions to read (shift = beta);
// both NULL: plain storage
__global__ __launch_bounds__(256) void bn_eval_affine_all_kernel(EvalAffineAll t, float eps, float* __restrict__ affine,
                                                                 const float* __restrict__ centres, float* __restrict__ centres_out) {
    const int l = blockIdx.x;
    for (int ch = threadIdx.x; ch < t.C[l]; ch += 256) {
        const float sc = t.gamma[l][ch] / sqrtf(t.rv[l][ch] + eps);
        const float rm = t.rm[l][ch];
        affine[(size_t)l * kAffStride + ch] = sc;
        if (centres) {
            affine[(size_t)l * kAffStride + kMaxC + ch] = t.beta[l][ch] - (rm - centres[(size_t)l * kMaxC + ch]) * sc;
        } else if (centres_out) {
            affine[(size_t)l * kAffStride + kMaxC + ch] = t.beta[l][ch];
            centres_out[(size_t)l * kMaxC + ch] = rm;
        } else {
            affine[(size_t)l * kAffStride + kMaxC + ch] = t.beta[l][ch] - rm * sc;
        }
    }
}

// per-column sum / sumsq partial rows of a stored [rows, C] tensor (fp32 parity path + tests)
template <typename T>
__global__ __launch_bounds__(256) void col_stats_kernel(const T* __restrict__ x, long rows, int C, float* __restrict__ stats) {
    __shared__ float ps[4][64], pq[4][64];
    const int c = threadIdx.x & 63, sl = threadIdx.x >> 6, ch = blockIdx.y * 64 + c;
    float s = 0.f, q = 0.f;
    if (ch < C) {
        for (long r = (long)blockIdx.x * 4 + sl; r < rows; r += (long)gridDim.x * 4) {
            const float v = ElemTraits<T>::to_f(x[r * C + ch]);
            s += v;
            q = fmaf(v, v, q);
        }
    }
    ps[sl][c] = s;
    pq[sl][c] = q;
    __syncthreads();
    if (sl == 0 && ch < C) {
        stats[((long)blockIdx.x * 2 + 0) * C + ch] = (ps[0][c] + ps[1][c]) + (ps[2][c] + ps[3][c]);
        stats[((long)blockIdx.x * 2 + 1) * C + ch] = (pq[0][c] + pq[1][c]) + (pq[2][c] + pq[3][c]);
    }
}

// ------------------------------------------------------------------------------------------------
// BN + ReLU + maxpool 3x3 stride 2 pad 1 (NHWC), 8 channels per thread
// ------------------------------------------------------------------------------------------------
// output rows per thread (round 5): R vertically adjacent outputs share input rows -- 3 (2 R + 1) taps for R outputs instead of 9 R, and
// (2 R + 1) / R instead of 3 input rows fetched per output row across the L2s (the counters had FETCH_SIZE at 1.5 x the input:
// consecutive output rows belong to workgroups on different XCDs)
constexpr int POOL_ROWS = 2;
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, T* __restrict__ y,
                                                              int B, int H, int W, int C) {
    constexpr int R = POOL_ROWS, NR = 2 * R + 1, NTAP = 3 * NR;
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1, CC = C / 8;
    const int Hq = (Ho + R - 1) / R;
    const long total = (long)B * Hq * Wo * CC;
    // (measured in round 3: an XCD-major block order -- consecutive 32-pixel blocks on one XCD so that the input row two output
    // rows share is fetched by one L2 instead of two -- made this kernel 7 % SLOWER (0.132 -> 0.142 ms); plain order kept)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % CC);
        const long p = i / CC;
        const int ox = (int)(p % Wo), oq = (int)((p / Wo) % Hq), b = (int)(p / ((long)Wo * Hq));
        const int oy = R * oq;
        float sc[8], sh[8], m[R][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc[e] = scale[cc * 8 + e]; sh[e] = shift[cc * 8 + e];
#pragma unroll
            for (int r = 0; r < R; ++r) m[r][e] = 0.f;                           // relu output >= 0
        }
        // all taps (input rows 2 oy - 1 .. 2 oy + 2 R - 1) are loaded from clamped (always valid) addresses before any is used; a
        // clamped tap repeats a pixel of the window it belongs to, which leaves the maximum unchanged -- no branch around a load
        // (branches made every tap wait for the previous one).  Output r's window is rows 2 r .. 2 r + 2 of the NR; where an output
        // does not exist (Ho not a multiple of R) its rows clamp into the image and its result is not stored
        constexpr int EPC = ElemTraits<T>::kPerChunk, NC = 8 / EPC;              // 8 channels = 1 (bf16) or 2 (fp32) chunks
        Chunk<T> tap[NTAP][NC];
        const T* src[NTAP];
#pragma unroll
        for (int ky = 0; ky < NR; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                // only row 0 can fall above the image (-> row 0, inside output 0's window); rows below it clamp to H - 1, which lies
                // inside the window of the last existing output
                const int yin = min(max(2 * oy - 1 + ky, 0), H - 1);
                const int xin = min(max(2 * ox - 1 + kx, 0), W - 1);
                src[ky * 3 + kx] = x + (((long)b * H + yin) * W + xin) * C + cc * 8;
            }
        // (the scheduler had sunk every tap's load next to its use -- nine s_waitcnt vmcnt(0), nine dependent round trips per
        // output, in the ISA -- although the source issued them together; the barriers pin "all addresses, all loads, then math")
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int q = 0; q < NC; ++q) tap[t][q].load(src[t] + q * EPC);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = fmaf(tap[t][e / EPC].get(e % EPC), sc[e], sh[e]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (t >= 6 * r && t < 6 * r + 9) m[r][e] = fmaxf(m[r][e], v);
            }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (oy + r < Ho) {
                T* dst = y + (((long)b * Ho + oy + r) * Wo + ox) * C + cc * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) dst[e] = ElemTraits<T>::from_f(m[r][e]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// out = relu(raw * scale + shift + identity),  identity = idn  or  idn * idn_scale + idn_shift
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bn_add_relu_kernel(const T* __restrict__ raw, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const T* __restrict__ idn,
                                                          const float* __restrict__ idn_scale,
                                                          const float* __restrict__ idn_shift, T* __restrict__ out,
                                                          long rows, int C) {
    // The grid stride (gridDim * 256 chunks) is a multiple of the chunks per row (chunk_keeping_grid below), so a thread
    // always lands on the same channel chunk: the per-channel affine is loaded once.
    constexpr int EPC = ElemTraits<T>::kPerChunk;
    const int CC = C / EPC;
    const long total = rows * CC;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (int)(i0 % CC) * EPC;
    // per-channel affines as 16-byte loads from unconditional addresses (a `cond ? p[i] : 1.f` per element made the compiler emit
    // one s_waitcnt vmcnt(0) per channel: eight dependent L2 round trips at the start of every workgroup)
    float sc[EPC], sh[EPC], isc[EPC], ish[EPC];
    const float* isp = idn_scale ? idn_scale : scale;
    const float* ihp = idn_scale ? idn_shift : shift;
#pragma unroll
    for (int v4 = 0; v4 < EPC / 4; ++v4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(scale + c + 4 * v4), b = *reinterpret_cast<const f32x4*>(shift + c + 4 * v4);
        const f32x4 ia = *reinterpret_cast<const f32x4*>(isp + c + 4 * v4), ib = *reinterpret_cast<const f32x4*>(ihp + c + 4 * v4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sc[4 * v4 + e] = a[e];
            sh[4 * v4 + e] = b[e];
            isc[4 * v4 + e] = idn_scale ? ia[e] : 1.f;
            ish[4 * v4 + e] = idn_scale ? ib[e] : 0.f;
        }
    }
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += 2 * stride) {          // two independent 16-B chunks in flight per thread
        const long j = i + stride;
        const bool has_j = j < total;
        Chunk<T> a0, d0, a1, d1, o;
        a0.load(raw + i * EPC);
        d0.load(idn + i * EPC);
        if (has_j) { a1.load(raw + j * EPC); d1.load(idn + j * EPC); }
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float v = fmaf(a0.get(e), sc[e], sh[e]);
            const float r = idn_scale ? fmaf(d0.get(e), isc[e], ish[e]) : d0.get(e);
            o.set(e, fmaxf(v + r, 0.f));
        }
        o.store(out + i * EPC);
        if (has_j) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float v = fmaf(a1.get(e), sc[e], sh[e]);
                const float r = idn_scale ? fmaf(d1.get(e), isc[e], ish[e]) : d1.get(e);
                o.set(e, fmaxf(v + r, 0.f));
            }
            o.store(out + j * EPC);
        }
    }
}

// y = relu(x * scale + shift) over [rows, C] (may run in place).  Used ahead of conv3: applying BatchNorm in the
// GEMM's operand load costs the affine once per 128-column tile of the output (2..16x redundant VALU work that
// also stalls the MFMA pipe), while this pass touches the narrow tensor exactly once.
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, T* __restrict__ y,
                                                            long rows, int C) {
    constexpr int EPC = ElemTraits<T>::kPerChunk;
    const int CC = C / EPC;
    const long total = rows * CC;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (int)(i0 % CC) * EPC;                 // fixed per thread: (grid * 256) % CC == 0 (chunk_keeping_grid)
    float sc[EPC], sh[EPC];
#pragma unroll
    for (int v4 = 0; v4 < EPC / 4; ++v4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(scale + c + 4 * v4), b = *reinterpret_cast<const f32x4*>(shift + c + 4 * v4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[4 * v4 + e] = a[e]; sh[4 * v4 + e] = b[e]; }
    }
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += 2 * stride) {
        const long j = i + stride;
        const bool has_j = j < total;
        Chunk<T> a0, a1, o;
        a0.load(x + i * EPC);
        if (has_j) a1.load(x + j * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, fmaxf(fmaf(a0.get(e), sc[e], sh[e]), 0.f));
        o.store(y + i * EPC);
        if (has_j) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, fmaxf(fmaf(a1.get(e), sc[e], sh[e]), 0.f));
            o.store(y + j * EPC);
        }
    }
}

// global average pool: [B, HW, C] -> [B, C] fp32
template <typename T>
__global__ __launch_bounds__(256) void avgpool_kernel(const T* __restrict__ x, float* __restrict__ out, int B, int HW, int C) {
    const long total = (long)B * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long b = i / C;
        const float acc = ordered_sum<8, float>(HW, [&](int p) { return ElemTraits<T>::to_f(x[(b * HW + p) * C + c]); });
        out[i] = acc / (float)HW;
    }
}

// ------------------------------------------------------------------------------------------------
// Grouped train-mode BatchNorm (linear-probe scoring, cvcl_resnext50_fwd_grouped): the batch is T consecutive groups of
// rows_g rows, and each group is normalised on its own mean and biased variance.  fp32 storage only (CVCL_F32, CVCL_F32X3).
// ------------------------------------------------------------------------------------------------
// partial moments of one row slice of one group -> part[T][S][2][C] = (slice mean, slice sum of squared deviations), centred
// two-pass: the slice's mean first, then sum (x - mean)^2 over the same rows (no E[x^2] - E[x]^2 cancellation).
// grid (S, T, C / 64); a thread owns 4 channels (one 16-byte load) of every 16th row of the slice.
__global__ __launch_bounds__(256) void bn_group_stats_kernel(const float* __restrict__ x, long rows_g, int C, int S,
                                                             float* __restrict__ part) {
    __shared__ f32x4 red[16][16];
    const int q = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int s = blockIdx.x, t = blockIdx.y, c0 = blockIdx.z * 64 + q * 4;
    const long r0 = rows_g * s / S, r1 = rows_g * (s + 1) / S;
    const float* xg = x + (long)t * rows_g * C + c0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long r = r0 + lane; r < r1; r += 16) acc += *reinterpret_cast<const f32x4*>(xg + r * C);
    red[lane][q] = acc;
    __syncthreads();
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i][q];                  // same fixed order in every thread of the column
    const float inv_n = 1.f / (float)(r1 - r0);
    const f32x4 mean = tot * inv_n;
    __syncthreads();                                                // every thread has read red before it is reused
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long r = r0 + lane; r < r1; r += 16) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(xg + r * C) - mean;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(d[k], d[k], acc[k]);
    }
    red[lane][q] = acc;
    __syncthreads();
    if (lane == 0) {
        f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i) m2 += red[i][q];
        float* p = part + ((long)t * S + s) * 2 * C + c0;
        *reinterpret_cast<f32x4*>(p) = mean;
        *reinterpret_cast<f32x4*>(p + C) = m2;
    }
}

// the S slices of every group merged in a fixed order in fp64 (Chan et al.: M2 = sum M2_s + n_s (mean_s - mean)^2), then the
// train-mode affine of nn.BatchNorm2d with the biased variance: scale = gamma / sqrt(var + eps), shift = beta - mean * scale.
// -> scale [T][C], shift [T][C]; grid (C / 256 rounded up, T)
__global__ __launch_bounds__(256) void bn_group_finalize_kernel(const float* __restrict__ part, long rows_g, int S, int C,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, float* __restrict__ scale, float* __restrict__ shift) {
    const int ch = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (ch >= C) return;
    const float* p = part + (long)t * S * 2 * C + ch;
    double mean = 0.0;
    for (int s = 0; s < S; ++s) {
        const double n = (double)(rows_g * (s + 1) / S - rows_g * s / S);
        mean += n * (double)p[(long)s * 2 * C];
    }
    mean /= (double)rows_g;
    double m2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double n = (double)(rows_g * (s + 1) / S - rows_g * s / S);
        const double d = (double)p[(long)s * 2 * C] - mean;
        m2 += (double)p[(long)s * 2 * C + C] + n * d * d;
    }
    const double var = m2 / (double)rows_g;
    const float sc = gamma[ch] / sqrtf((float)var + eps);
    scale[(long)t * C + ch] = sc;
    shift[(long)t * C + ch] = beta[ch] - (float)mean * sc;
}

// y = relu(x * scale[g] + shift[g]) over [rows, C], g = row / rows_g (may run in place)
__global__ __launch_bounds__(256) void bn_group_relu_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y, long rows,
                                                            int C, long rows_g) {
    const int CC = C / 4;
    const long total = rows * CC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / CC;
        const long a = r / rows_g * C + (i - r * CC) * 4;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + a), sh = *reinterpret_cast<const f32x4*>(shift + a);
        f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(fmaf(v[k], sc[k], sh[k]), 0.f);
        *reinterpret_cast<f32x4*>(y + i * 4) = v;
    }
}

// out = relu(raw * scale[g] + shift[g] + identity), identity = idn or idn * idn_scale[g] + idn_shift[g]; g = row / rows_g
__global__ __launch_bounds__(256) void bn_group_add_relu_kernel(const float* __restrict__ raw, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* __restrict__ idn,
                                                                const float* __restrict__ idn_scale,
                                                                const float* __restrict__ idn_shift, float* __restrict__ out,
                                                                long rows, int C, long rows_g) {
    const int CC = C / 4;
    const long total = rows * CC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / CC;
        const long a = r / rows_g * C + (i - r * CC) * 4;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + a), sh = *reinterpret_cast<const f32x4*>(shift + a);
        const f32x4 v = *reinterpret_cast<const f32x4*>(raw + i * 4);
        f32x4 d = *reinterpret_cast<const f32x4*>(idn + i * 4);
        if (idn_scale) {
            const f32x4 isc = *reinterpret_cast<const f32x4*>(idn_scale + a), ish = *reinterpret_cast<const f32x4*>(idn_shift + a);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = fmaf(d[k], isc[k], ish[k]);
        }
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaxf(fmaf(v[k], sc[k], sh[k]) + d[k], 0.f);
        *reinterpret_cast<f32x4*>(out + i * 4) = o;
    }
}

// relu(bn(x)) then maxpool 3x3/2 pad 1: [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C], image b normalised with group b / G's affine.
// The ReLU output is >= 0 and every window holds at least one pixel, so a maximum started at 0 over the in-image taps equals
// torch's -inf padding.
__global__ __launch_bounds__(256) void bn_group_relu_maxpool_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, float* __restrict__ y,
                                                                    int B, int H, int W, int C, int G) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, CC = C / 4;
    const long total = (long)B * Ho * Wo * CC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % CC);
        const long p = i / CC;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
        const long a = (long)(b / G) * C + cc * 4;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + a), sh = *reinterpret_cast<const f32x4*>(shift + a);
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < 3; ++ky) {
            const int yin = 2 * oy - 1 + ky;
            if (yin < 0 || yin >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xin = 2 * ox - 1 + kx;
                if (xin < 0 || xin >= W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + yin) * W + xin) * C + cc * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = fmaxf(m[k], fmaf(v[k], sc[k], sh[k]));
            }
        }
        *reinterpret_cast<f32x4*>(y + p * C + cc * 4) = m;
    }
}

}  // namespace

// ================================================================================================
// C ABI, and the launchers of the trunk walk (cvcl_common.h)
// ================================================================================================
int cvcl_bn_finalize_launch(const float* stats, int rows, long count, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                            float eps, float* scale, float* shift, int C, float* moments, int moments_ld, const float* centre,
                            void* stream) {
    CVCL_CHECK_ARG(stats && gamma && beta && scale && shift && rows > 0 && count > 0 && C > 0, "cvcl_bn_finalize: bad args");
    CvclProfScope prof(stream, CVCL_K_BN_FINALIZE);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cvcl_div_up(C, 16)), dim3(1024), 0, (hipStream_t)stream, stats, rows,
                       (double)count, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, scale,
                       shift, C, moments, moments_ld, centre);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_bn_finalize(const float* stats, int rows, long count, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                                float eps, float* scale, float* shift, const float* centre, int C, void* stream) {
    return cvcl_bn_finalize_launch(stats, rows, count, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                                   scale, shift, C, nullptr, 0, centre, stream);
}

extern "C" int cvcl_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, float* scale, float* shift, const float* centre, int C,
                                   void* stream) {
    CVCL_CHECK_ARG(gamma && beta && running_mean && running_var && scale && shift && C > 0, "cvcl_bn_eval_affine: bad args");
    CvclProfScope prof(stream, CVCL_K_BN_FINALIZE);
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(cvcl_div_up(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                       running_mean, running_var, eps, scale, shift, centre, C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_col_stats_rows(long rows) {
    long g = (rows + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > 256 ? 256 : g);
}

extern "C" int cvcl_col_stats(int dtype, const void* x, long rows, int C, float* stats, int stats_rows, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_col_stats");
    dtype = cvcl_storage_dtype(dtype);
    CVCL_CHECK_ARG(x && stats && rows > 0 && C > 0, "cvcl_col_stats: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const int g = cvcl_col_stats_rows(rows);
    CVCL_CHECK_ARG(stats_rows >= g, "cvcl_col_stats: stats_rows %d < %d", stats_rows, g);
    dim3 grid(g, cvcl_div_up(C, 64));
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(col_stats_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, rows, C, stats);
    else
        hipLaunchKernelGGL(col_stats_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, rows, C, stats);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_bn_relu_maxpool(int dtype, const void* x, const float* scale, const float* shift, void* y, int B,
                                    int H, int W, int C, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_bn_relu_maxpool");
    dtype = cvcl_storage_dtype(dtype);
    CVCL_CHECK_ARG(x && scale && shift && y && C % 8 == 0, "cvcl_bn_relu_maxpool: bad args");
    CvclProfScope prof(stream, CVCL_K_MAXPOOL);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = (long)B * ((Ho + POOL_ROWS - 1) / POOL_ROWS) * Wo * (C / 8);          // a thread owns POOL_ROWS output rows
    const int grid = cvcl_grid(total, 256, 8192);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(bn_relu_maxpool_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           (const float*)x, scale, shift, (float*)y, B, H, W, C);
    else
        hipLaunchKernelGGL(bn_relu_maxpool_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, scale, shift, (bf16_t*)y, B, H, W, C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// Grid of bn_add_relu_kernel and bn_relu_apply_kernel over rows x cc 16-byte chunks (cc per row).  Their threads load the affine of
// their channel chunk once, so a thread has to stay on that chunk across its iterations: (grid * 256) % cc == 0, i.e. the grid is a
// multiple of cc / gcd(cc, 256).
static int chunk_keeping_grid(long rows, int cc) {
    int g256 = cc, t256 = 256;
    while (t256) { const int r = g256 % t256; g256 = t256; t256 = r; }      // gcd(cc, 256)
    const int mult = cc / g256;
    const int grid = cvcl_grid(rows * (long)cc, 256 * 4, 16384);
    return (grid + mult - 1) / mult * mult;
}

extern "C" int cvcl_bn_add_relu(int dtype, const void* raw, const float* scale, const float* shift, const void* idn,
                                const float* idn_scale, const float* idn_shift, void* out, long rows, int C, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_bn_add_relu");
    dtype = cvcl_storage_dtype(dtype);
    CVCL_CHECK_ARG(raw && scale && shift && idn && out && rows > 0, "cvcl_bn_add_relu: bad args");
    CvclProfScope prof(stream, CVCL_K_BN_ADD_RELU);
    CVCL_CHECK_ARG((idn_scale == nullptr) == (idn_shift == nullptr), "cvcl_bn_add_relu: idn_scale/idn_shift pair");
    const int epc = dtype == CVCL_F32 ? 4 : 8;
    CVCL_CHECK_ARG(C % epc == 0, "cvcl_bn_add_relu: C must be a multiple of %d", epc);
    hipStream_t s = (hipStream_t)stream;
    const int grid = chunk_keeping_grid(rows, C / epc);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(bn_add_relu_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)raw,
                           scale, shift, (const float*)idn, idn_scale, idn_shift, (float*)out, rows, C);
    else
        hipLaunchKernelGGL(bn_add_relu_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)raw,
                           scale, shift, (const bf16_t*)idn, idn_scale, idn_shift, (bf16_t*)out, rows, C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_bn_relu_apply(int dtype, const void* x, const float* scale, const float* shift, void* y, long rows,
                                  int C, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_bn_relu_apply");
    dtype = cvcl_storage_dtype(dtype);
    CVCL_CHECK_ARG(x && scale && shift && y && rows > 0, "cvcl_bn_relu_apply: bad args");
    CvclProfScope prof(stream, CVCL_K_BN_APPLY);
    const int epc = dtype == CVCL_F32 ? 4 : 8;
    CVCL_CHECK_ARG(C % epc == 0, "cvcl_bn_relu_apply: C must be a multiple of %d", epc);
    const int grid = chunk_keeping_grid(rows, C / epc);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(bn_relu_apply_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, scale,
                           shift, (float*)y, rows, C);
    else
        hipLaunchKernelGGL(bn_relu_apply_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           scale, shift, (bf16_t*)y, rows, C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_avgpool(int dtype, const void* x, float* out, int B, int HW, int C, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_avgpool");
    dtype = cvcl_storage_dtype(dtype);
    CVCL_CHECK_ARG(x && out && B > 0 && HW > 0 && C > 0, "cvcl_avgpool: bad args");
    CvclProfScope prof(stream, CVCL_K_AVGPOOL);
    if (dtype == CVCL_F32)
        hipLaunchKernelGGL(avgpool_kernel<float>, dim3(cvcl_grid((long)B * C, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const float*)x, out, B, HW, C);
    else
        hipLaunchKernelGGL(avgpool_kernel<bf16_t>, dim3(cvcl_grid((long)B * C, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, out, B, HW, C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// ---- the one-launch passes over the whole trunk (the callers in csrc/resnext.hip fill and check the layer tables) ----
int cvcl_bn_eval_affine_all(const EvalAffineAll& t, float eps, float* affine, const float* centres, float* centres_out, void* stream) {
    CvclProfScope prof(stream, CVCL_K_BN_FINALIZE);
    hipLaunchKernelGGL(bn_eval_affine_all_kernel, dim3(kTrunkLayers), dim3(256), 0, (hipStream_t)stream, t, eps, affine, centres,
                       centres_out);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_bn_apply_moments_all(const ApplyMomentsAll& t, const float* moments, float momentum, void* stream) {
    CvclProfScope prof(stream, CVCL_K_BN_FINALIZE);
    hipLaunchKernelGGL(bn_apply_moments_kernel, dim3(kTrunkLayers), dim3(256), 0, (hipStream_t)stream, t, moments, momentum);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// ---- the grouped train-mode pass (cvcl_resnext50_fwd_grouped) ----
// row slices per group for bn_group_stats: about 2048 workgroups in all, >= 64 rows a slice, at most 64 slices
static int group_slices(int T, long rows_g, int C) {
    long s = 2048 / ((long)T * (C / 64));
    if (s > 64) s = 64;
    if (s > rows_g / 64) s = rows_g / 64;
    return s < 1 ? 1 : (int)s;
}
// part[T][S][2][C] holds 128 T S (C / 64) floats; group_slices keeps T S (C / 64) <= max(2048, 32 T)
size_t cvcl_bn_group_part_floats(int T) { return (size_t)128 * std::max<size_t>(2048, (size_t)32 * T); }

// a layer's raw output y ([T groups of rows_g rows, C]) -> its per-group affine in a
int cvcl_bn_group_affine(const float* y, int T, long rows_g, int C, const float* gamma, const float* beta, float eps, float* part, float* a,
                         void* stream) {
    const int S = group_slices(T, rows_g, C);
    {
        CvclProfScope prof(stream, CVCL_K_OTHER);
        hipLaunchKernelGGL(bn_group_stats_kernel, dim3(S, T, C / 64), dim3(256), 0, (hipStream_t)stream, y, rows_g, C, S, part);
        CVCL_LAUNCH_CHECK();
    }
    CvclProfScope prof(stream, CVCL_K_BN_FINALIZE);
    hipLaunchKernelGGL(bn_group_finalize_kernel, dim3(cvcl_div_up(C, 256), T), dim3(256), 0, (hipStream_t)stream, part, rows_g, S, C,
                       gamma, beta, eps, a, a + (size_t)T * C);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_bn_group_relu(float* x, const float* a, int T, long rows, int C, long rows_g, void* stream) {
    CvclProfScope prof(stream, CVCL_K_BN_APPLY);
    hipLaunchKernelGGL(bn_group_relu_kernel, dim3(cvcl_grid(rows * (C / 4), 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, a,
                       a + (size_t)T * C, x, rows, C, rows_g);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_bn_group_add_relu(const float* raw, const float* a, const float* idn, const float* idn_a, float* out, int T, long rows, int C,
                           long rows_g, void* stream) {
    CvclProfScope prof(stream, CVCL_K_BN_ADD_RELU);
    hipLaunchKernelGGL(bn_group_add_relu_kernel, dim3(cvcl_grid(rows * (C / 4), 256, 16384)), dim3(256), 0, (hipStream_t)stream, raw, a,
                       a + (size_t)T * C, idn, idn_a, idn_a ? idn_a + (size_t)T * C : nullptr, out, rows, C, rows_g);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_bn_group_relu_maxpool(const float* x, const float* a, float* y, int B, int H, int W, int C, int group, void* stream) {
    CvclProfScope prof(stream, CVCL_K_MAXPOOL);
    const long total = (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (C / 4);
    hipLaunchKernelGGL(bn_group_relu_maxpool_kernel, dim3(cvcl_grid(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, a,
                       a + (size_t)(B / group) * C, y, B, H, W, C, group);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
