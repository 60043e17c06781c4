// The 7x7 stride-2 stem convolution of the ResNeXt-50 trunk for gfx950 (reference: conv1 of torchvision.models.resnext50_32x4d, and
// conv1 -> bn1 -> relu -> maxpool of ResNet.forward for the fused form, reached at multimodal/multimodal.py:101 through
// VisionEncoder.forward).  NCHW fp32 image -> NHWC raw output (before BatchNorm, csrc/bn.hip) with its per-channel statistics rows.
//
//   stem_mfma_kernel       bf16: MFMA 16x16x32, B-operand gathered straight from an LDS image patch
//                          (k ordered (c, ky, kx padded to 8): 8 consecutive k = 8 consecutive pixels; pack_stem_kernel's layout)
//   stem_pool_mfma_kernel  bf16: the same convolution recomputed with bn1 + relu + maxpool applied out of LDS (cvcl_stem_pool)
//   stem_tiled_f32_kernel, stem_direct_f32_kernel
//                          fp32 (parity mode): VALU kernels with identical semantics; their statistics come from cvcl_col_stats
// CVCL_F32X3 goes to csrc/conv_split.hip.
#include "cvcl_common.h"

namespace {

// stem: [64][3][7][7] -> bf16 [4 ntile][6 kstep][16 n][32 k], k = kblock*8 + kx, r = 4*kstep + kblock = c*7 + ky
__global__ void pack_stem_kernel(const float* __restrict__ w, bf16_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * 6 * 16 * 32) return;
    const int k = i & 31, n = (i >> 5) & 15, ks = (i >> 9) % 6, nt = i / (6 * 512);
    const int r = 4 * ks + (k >> 3), kx = k & 7;
    float v = 0.f;
    if (r < 21 && kx < 7) {
        const int c = r / 7, ky = r % 7;
        v = w[((nt * 16 + n) * 3 + c) * 49 + ky * 7 + kx];
    }
    out[i] = (bf16_t)v;
}

// ------------------------------------------------------------------------------------------------
// stem 7x7 stride 2 pad 3, NCHW fp32 image -> NHWC raw                       (bf16, MFMA)
// ------------------------------------------------------------------------------------------------
constexpr int STEM_TH = 4;                 // output rows per work item
constexpr int STEM_ROWS = 2 * STEM_TH + 5; // input rows per channel
constexpr int STEM_PITCH = 144;            // dwords per patch row (288 bf16 >= 224 + 6 + 8 slack); 144 % 32 == 16
constexpr int STEM_OPITCH = 144;           // bytes per pixel of a wave's output slot (128 + 16 pad)

__global__ __launch_bounds__(256, 2) void stem_mfma_kernel(const float* __restrict__ x, const bf16_t* __restrict__ wp,
                                                        bf16_t* __restrict__ y, float* __restrict__ stats,
                                                        const float* __restrict__ centre, int B, int Hin, int Win) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned int* patch = (unsigned int*)smem;                 // [3*STEM_ROWS][STEM_PITCH] dwords (2 bf16 each)
    const int Ho = Hin / 2, Wo = Win / 2;
    const int bands = cvcl_div_up(Ho, STEM_TH);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pix = lane & 15, kb = lane >> 4;

    bf16x8 wf[4][6];                                           // all 64 output channels' weights, register resident
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int ks = 0; ks < 6; ++ks)
            wf[nt][ks] = *reinterpret_cast<const bf16x8*>(wp + ((nt * 6 + ks) * 16 + pix) * 32 + kb * 8);

    f32x2 ssum[4][2], ssq[4][2];                              // (channel pairs: packed fp32)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { ssum[a][b] = f32x2{0.f, 0.f}; ssq[a][b] = f32x2{0.f, 0.f}; }

    const int mtiles_per_row = cvcl_div_up(Wo, 16);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // per-lane constants of the multiply loop: patch row (dwords) of k step ks -- k = 4 ks + kb -> (channel, ky), padded k at 20
    int koff[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
        const int r = min(4 * ks + kb, 20);
        const int c = r / 7, ky = r - c * 7;
        koff[ks] = (c * STEM_ROWS + ky) * STEM_PITCH;
    }
    for (int i = tid; i < 3 * STEM_ROWS * STEM_PITCH; i += 256) patch[i] = 0u;       // pad columns stay zero for good
    char* wst = smem + 3 * STEM_ROWS * STEM_PITCH * 4 + wave * (16 * STEM_OPITCH);  // this wave's output slot: 16 pixels
    // centred storage: the accumulators start at -centre[channel] (64 floats in LDS behind the output slots, re-read per tile:
    // the weights already hold 96 registers)
    float* cen = reinterpret_cast<float*>(smem + 3 * STEM_ROWS * STEM_PITCH * 4 + 4 * 16 * STEM_OPITCH);
    if (tid < 64) cen[tid] = centre ? -centre[tid] : 0.f;                           // (visible after the first item's barrier)
    // (XCD-major item order, as in gconv_mfma_kernel: adjacent bands of an image share 5 of their 13 input rows -- 0.247 GB read for
    // a 0.154 GB input in the plain order; time-neutral for this kernel, the traffic is what it saves)
    const int bx = (gridDim.x & 7) == 0 ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
    for (int item = bx; item < B * bands; item += gridDim.x) {
        const int b = item / bands, band = item - b * bands;
        const int oy0 = band * STEM_TH;
        __syncthreads();
        // stage: rows (c, iy) <- x[b][c][2*oy0 - 3 + iy][*] as bf16 at columns x + 3 (the 3 + slack pad columns on either side were
        // zeroed once and are never written).  Slot s of a wave is patch row 4 s + wave, a lane is one 16-byte vector of that row
        // (Win / 4 <= 64 of them): the row, its channel, input row and validity are wave-uniform scalars -- no per-thread index
        // arithmetic (the flat index form spent two runtime divisions per slot and phase).  All of a batch's loads are issued
        // before the first LDS write; rows outside the image are staged as zeros.
        {
            constexpr int NROW = 3 * STEM_ROWS, NV = 5;          // two batches of 5 slots: 10 x 4 rows >= 39
            const int vec_per_row = Win / 4, jl = min(lane, vec_per_row - 1);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 v[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int r = min((half * NV + i) * 4 + wave_u, NROW - 1);
                    const int c = r / STEM_ROWS, iy = r - c * STEM_ROWS;
                    const int yin = min(max(2 * oy0 - 3 + iy, 0), Hin - 1);
                    v[i] = *reinterpret_cast<const f32x4*>(x + (((long)b * 3 + c) * Hin + yin) * Win + 4 * jl);
                }
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int r = (half * NV + i) * 4 + wave_u;
                    const int iy = r % STEM_ROWS, yin = 2 * oy0 - 3 + iy;
                    if (r < NROW && lane < vec_per_row) {
                        const bool ok = yin >= 0 && yin < Hin;
                        const unsigned u01 = ok ? round2(f32x2{v[i][0], v[i][1]}) : 0u, u23 = ok ? round2(f32x2{v[i][2], v[i][3]}) : 0u;
                        // four pixels from padded column 4 lane + 3 (odd): 2 + 4 + 2 bytes
                        char* dst = reinterpret_cast<char*>(patch + r * STEM_PITCH) + 8 * lane + 6;
                        *reinterpret_cast<unsigned short*>(dst) = (unsigned short)u01;
                        *reinterpret_cast<unsigned*>(dst + 2) = (u01 >> 16) | (u23 << 16);
                        *reinterpret_cast<unsigned short*>(dst + 6) = (unsigned short)(u23 >> 16);
                    }
                }
            }
        }
        __syncthreads();
        // m-tiles of the band in row-major order, wave w takes w, w + 4, ...: (row, tile in row) advance as scalars
        int ty = 0, tx = wave_u;
        while (tx >= mtiles_per_row) { tx -= mtiles_per_row; ++ty; }
        while (ty < STEM_TH) {
            const int ox0 = tx * 16;
            const int oy = oy0 + ty, ox = ox0 + pix;
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = *reinterpret_cast<const f32x4*>(cen + nt * 16 + kb * 4);
            const unsigned int* row0 = patch + 2 * ty * STEM_PITCH + (ox < Wo ? ox : 0);
#pragma unroll
            for (int ks = 0; ks < 6; ++ks) {
                const unsigned int* src = row0 + koff[ks];
                u32x4 raw = {src[0], src[1], src[2], src[3]};      // 8 consecutive input pixels (kx = 0..7)
                const bf16x8 bfrag = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][ks], bfrag, acc[nt], 0, 0, 0);
            }
            // the tile (16 pixels x 64 channels) goes through a wave-private LDS slot so that it leaves as full 128-byte pixel rows
            // (16 B per lane) instead of 8-byte pieces in the MFMA layout
            const bool inside = oy < Ho && ox < Wo;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const u32x2 o = {round2(f32x2{acc[nt][0], acc[nt][1]}), round2(f32x2{acc[nt][2], acc[nt][3]})};
                *reinterpret_cast<u32x2*>(wst + pix * STEM_OPITCH + nt * 32 + kb * 8) = o;
                if (inside) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const f32x2 sv = widen2(o[e]);
                        ssum[nt][e] += sv;
                        ssq[nt][e] = __builtin_elementwise_fma(sv, sv, ssq[nt][e]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            if (oy < Ho && y) {                                   // (y == NULL: statistics only -- the fused stem below recomputes the tile)
                bf16_t* drow = y + (((long)b * Ho + oy) * Wo + ox0) * 64 + (lane & 7) * 8;
#pragma unroll
                for (int rd = 0; rd < 2; ++rd) {
                    const int px = (lane >> 3) + 8 * rd;
                    const u32x4 v = *reinterpret_cast<const u32x4*>(wst + px * STEM_OPITCH + (lane & 7) * 16);
                    if (ox0 + px < Wo) *reinterpret_cast<u32x4*>(drow + (long)px * 64) = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            tx += 4;
            while (tx >= mtiles_per_row) { tx -= mtiles_per_row; ++ty; }
        }
    }
    // statistics: reduce over the 16 pixel lanes, then over the 4 waves; channel = nt*16 + kb*4 + e
    __syncthreads();
    float* red = (float*)smem;                                    // [4 waves][2][64]
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = ssum[nt][e >> 1][e & 1], q = ssq[nt][e >> 1][e & 1];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
            if (pix == 0) {
                red[(wave * 2 + 0) * 64 + nt * 16 + kb * 4 + e] = s;
                red[(wave * 2 + 1) * 64 + nt * 16 + kb * 4 + e] = q;
            }
        }
    __syncthreads();
    if (tid < 128) {
        const int which = tid >> 6, c = tid & 63;
        const float v = (red[(0 * 2 + which) * 64 + c] + red[(1 * 2 + which) * 64 + c]) +
                        (red[(2 * 2 + which) * 64 + c] + red[(3 * 2 + which) * 64 + c]);
        stats[((long)blockIdx.x * 2 + which) * 64 + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// stem 7x7 stride 2 + BatchNorm + ReLU + maxpool 3x3 stride 2 pad 1 in ONE pass (round 5; torchvision ResNet.forward
// conv1 -> bn1 -> relu -> maxpool, reached from multimodal/multimodal.py:101): NCHW fp32 image -> NHWC bf16 [B, H/4, W/4, 64].
// The raw stem output [B, 112, 112, 64] (411 MB at B = 256) is never written: train mode runs stem_mfma_kernel with y = NULL first
// (statistics only), bn_finalize, then this kernel RECOMPUTES the convolution (it is 30 GFLOP) and pools it out of LDS --
// 0.57 + 0.72 GB of traffic become 0.15 + 0.26 GB.  Bit-identical to the two-pass form: the same MFMA sequence per output, the same
// rounding of the raw value to bf16 before the affine, and round(max) == max(round) on the non-negative post-ReLU values.
// One 512-thread workgroup per CU; an item = STEMP_TP pooled rows of one image = 2 TP + 1 convolution rows (the first one shared
// with the previous item: 25 % recomputation at TP = 2) = 4 TP + 7 input rows per channel.  Convolution tiles (16 pixels x 64
// channels, 24 MFMAs) are dealt to the 8 waves and land, normalised, in an LDS band [conv row][pixel + 1][64 channels]; after a
// barrier every thread takes (pooled pixel, 8 channels) units: nine 16-byte LDS reads, packed integer maxima, one 16-byte store.
constexpr int STEMP_TP = 2;
constexpr int STEMP_CR = 2 * STEMP_TP + 1;             // convolution rows per item
constexpr int STEMP_ROWS = 2 * STEMP_CR + 5;           // input rows per channel
constexpr int STEMP_BW = 128;                          // band row width in pixels (column 0 = the left padding column)
// bytes of the band [STEMP_CR][STEMP_BW][64] bf16 plus ONE pixel of slack.  A convolution tile stores its pixel ox at band column
// ox + 1, and at 114 <= Wo <= 126 (W = 228 .. 252) the row has 8 tiles: lane 15 of the last one (a padding pixel, it stores zeros)
// lands on column STEMP_BW = column 0 of the next band row (a padding column: zero anyway) and, in the last band row, on the 128
// bytes behind the band.  Without the slack those were -centre[0..31], which every later tile starts its accumulators from.
constexpr int STEMP_BAND_BYTES = (STEMP_CR * STEMP_BW + 1) * 128;
__global__ __launch_bounds__(512, 1) void stem_pool_mfma_kernel(const float* __restrict__ x, const bf16_t* __restrict__ wp,
                                                                bf16_t* __restrict__ y, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* __restrict__ centre,
                                                                int B, int Hin, int Win) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned int* patch = (unsigned int*)smem;                 // [3 * STEMP_ROWS][STEM_PITCH] dwords (2 bf16 each)
    char* band = smem + 3 * STEMP_ROWS * STEM_PITCH * 4;       // [STEMP_CR][STEMP_BW][64] bf16
    float* cen = reinterpret_cast<float*>(band + STEMP_BAND_BYTES);               // [64] -centre | [64] scale | [64] shift
    const int Ho = Hin / 2, Wo = Win / 2;
    const int Hp = (Ho - 1) / 2 + 1, Wp = (Wo - 1) / 2 + 1;
    const int bands = cvcl_div_up(Hp, STEMP_TP);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pix = lane & 15, kb = lane >> 4;

    bf16x8 wf[4][6];                                           // all 64 output channels' weights, register resident
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int ks = 0; ks < 6; ++ks)
            wf[nt][ks] = *reinterpret_cast<const bf16x8*>(wp + ((nt * 6 + ks) * 16 + pix) * 32 + kb * 8);
    const int mtiles_per_row = cvcl_div_up(Wo, 16);
    int koff[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
        const int r = min(4 * ks + kb, 20);
        const int c = r / 7, ky = r - c * 7;
        koff[ks] = (c * STEMP_ROWS + ky) * STEM_PITCH;
    }
    for (int i = tid; i < 3 * STEMP_ROWS * STEM_PITCH; i += 512) patch[i] = 0u;       // pad columns stay zero for good
    for (int i = tid; i < STEMP_CR * STEMP_BW * 32; i += 512) reinterpret_cast<unsigned*>(band)[i] = 0u;   // (padding columns: never rewritten)
    if (tid < 64) {
        cen[tid] = centre ? -centre[tid] : 0.f;
        cen[64 + tid] = scale[tid];
        cen[128 + tid] = shift[tid];
    }
    const int bx = (gridDim.x & 7) == 0 ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
    for (int item = bx; item < B * bands; item += gridDim.x) {
        const int b = item / bands, bnd = item - b * bands;
        const int p0 = bnd * STEMP_TP;
        const int oy_first = 2 * p0 - 1;                      // convolution row of band row 0 (-1 for the first item: padding)
        // ---- stage: rows (c, iy) <- x[b][c][2 oy_first - 3 + iy][*] as bf16 at columns x + 3 (see stem_mfma_kernel) ----
        {
            constexpr int NROW = 3 * STEMP_ROWS, NV = (NROW + 15) / 16;      // 8 waves x 2 batches x NV slots >= NROW
            const int vec_per_row = Win / 4, jl = min(lane, vec_per_row - 1);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 v[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int r = min((half * NV + i) * 8 + wave_u, NROW - 1);
                    const int c = r / STEMP_ROWS, iy = r - c * STEMP_ROWS;
                    const int yin = min(max(2 * oy_first - 3 + iy, 0), Hin - 1);
                    v[i] = *reinterpret_cast<const f32x4*>(x + (((long)b * 3 + c) * Hin + yin) * Win + 4 * jl);
                }
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int r = (half * NV + i) * 8 + wave_u;
                    const int iy = r % STEMP_ROWS, yin = 2 * oy_first - 3 + iy;
                    if (r < NROW && lane < vec_per_row) {
                        const bool ok = yin >= 0 && yin < Hin;
                        const unsigned u01 = ok ? round2(f32x2{v[i][0], v[i][1]}) : 0u, u23 = ok ? round2(f32x2{v[i][2], v[i][3]}) : 0u;
                        char* dst = reinterpret_cast<char*>(patch + r * STEM_PITCH) + 8 * lane + 6;
                        *reinterpret_cast<unsigned short*>(dst) = (unsigned short)u01;
                        *reinterpret_cast<unsigned*>(dst + 2) = (u01 >> 16) | (u23 << 16);
                        *reinterpret_cast<unsigned short*>(dst + 6) = (unsigned short)(u23 >> 16);
                    }
                }
            }
        }
        __syncthreads();
        // ---- convolution tiles of the band's STEMP_CR rows: wave w takes tiles w, w + 8, ... (row-major) ----
        for (int t = wave_u; t < STEMP_CR * mtiles_per_row; t += 8) {
            const int ty = t / mtiles_per_row, tx = t - ty * mtiles_per_row;
            const int ox0 = tx * 16, ox = ox0 + pix;
            const int oy = oy_first + ty;
            char* brow = band + (ty * STEMP_BW + ox + 1) * 128 + kb * 8;
            if (oy < 0 || oy >= Ho) {                          // a padding row of the pooling window: zeros (post-ReLU domain)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<u32x2*>(brow + nt * 32) = u32x2{0u, 0u};
                continue;
            }
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = *reinterpret_cast<const f32x4*>(cen + nt * 16 + kb * 4);
            const unsigned int* row0 = patch + 2 * ty * STEM_PITCH + (ox < Wo ? ox : 0);
#pragma unroll
            for (int ks = 0; ks < 6; ++ks) {
                const unsigned int* src = row0 + koff[ks];
                u32x4 raw = {src[0], src[1], src[2], src[3]};
                const bf16x8 bfrag = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][ks], bfrag, acc[nt], 0, 0, 0);
            }
            const bool inside = ox < Wo;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                // what the two-pass form stores, then what bn_relu_maxpool computes from it: relu(raw_bf16 * scale + shift)
                const u32x2 o = {round2(f32x2{acc[nt][0], acc[nt][1]}), round2(f32x2{acc[nt][2], acc[nt][3]})};
                const f32x4 sc4 = *reinterpret_cast<const f32x4*>(cen + 64 + nt * 16 + kb * 4);
                const f32x4 sh4 = *reinterpret_cast<const f32x4*>(cen + 128 + nt * 16 + kb * 4);
                const f32x2 r01 = widen2(o[0]), r23 = widen2(o[1]);
                const f32x2 v01 = {fmaxf(fmaf(r01[0], sc4[0], sh4[0]), 0.f), fmaxf(fmaf(r01[1], sc4[1], sh4[1]), 0.f)};
                const f32x2 v23 = {fmaxf(fmaf(r23[0], sc4[2], sh4[2]), 0.f), fmaxf(fmaf(r23[1], sc4[3], sh4[3]), 0.f)};
                *reinterpret_cast<u32x2*>(brow + nt * 32) = inside ? u32x2{round2(v01), round2(v23)} : u32x2{0u, 0u};
            }
        }
        __syncthreads();
        // ---- pool: (pooled row pr, pooled pixel pc, 8-channel chunk c8) units; band row 2 pr + dy, band column 2 pc + dx ----
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
        for (int u = tid; u < STEMP_TP * Wp * 8; u += 512) {
            const int c8 = u & 7, q = u >> 3;
            const int pr = q / Wp, pc = q - pr * Wp;
            if (p0 + pr >= Hp) continue;
            const char* src = band + ((2 * pr) * STEMP_BW + 2 * pc) * 128 + c8 * 16;
            u16x8 m = *reinterpret_cast<const u16x8*>(src);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    if (dy == 0 && dx == 0) continue;
                    // (2 pc + dx <= Wo + 1 < STEMP_BW; the band's right padding columns are zero)
                    m = __builtin_elementwise_max(m, *reinterpret_cast<const u16x8*>(src + (dy * STEMP_BW + dx) * 128));
                }
            *reinterpret_cast<u16x8*>(y + (((long)b * Hp + p0 + pr) * Wp + pc) * 64 + c8 * 8) = m;
        }
        // (the next item's staging touches only the patch, which nobody reads after the barrier above; its convolution phase
        // rewrites the band behind the staging barrier, which every thread reaches with its pooling done)
    }
}

// fp32 parity path: direct convolution, one thread per (pixel, output channel); weights in OIHW
__global__ __launch_bounds__(256) void stem_direct_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              float* __restrict__ y, const float* __restrict__ centre,
                                                              int B, int Hin, int Win) {
    const int Ho = Hin / 2, Wo = Win / 2;
    const long total = (long)B * Ho * Wo * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i & 63);
        const long p = i >> 6;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
        float acc = centre ? -centre[co] : 0.f;
        for (int c = 0; c < 3; ++c)
            for (int ky = 0; ky < 7; ++ky) {
                const int yin = 2 * oy - 3 + ky;
                if (yin < 0 || yin >= Hin) continue;
                for (int kx = 0; kx < 7; ++kx) {
                    const int xin = 2 * ox - 3 + kx;
                    if (xin < 0 || xin >= Win) continue;
                    acc = fmaf(x[(((long)b * 3 + c) * Hin + yin) * Win + xin], w[((co * 3 + c) * 7 + ky) * 7 + kx], acc);
                }
            }
        y[i] = acc;
    }
}

// fp32 parity path, LDS-tiled (the direct kernel above stays as the fallback for shapes whose band does not fit): one workgroup =
// one band of TH output rows of one image.  The band's input rows (zero padding included) are staged per channel in LDS, the
// weights transposed to [tap][co]; a wave then takes (16-channel chunk, 64 output pixels) units: lane = pixel, 16 accumulators,
// per tap one LDS read of the input value and 16 FMAs against wave-uniform weights (broadcast 16-byte LDS reads).
__global__ __launch_bounds__(256) void stem_tiled_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             float* __restrict__ y, const float* __restrict__ centre,
                                                             int B, int Hin, int Win, int TH, int bands) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    const int Ho = Hin / 2, Wo = Win / 2;
    const int Wp = Win + 6, rows_in = 2 * TH + 5, plane = rows_in * Wp;
    float* ws = smf;                                  // [147][64]
    float* cs = ws + 147 * 64;                        // [64]  -centre
    float* xs = cs + 64;                              // [3][plane]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < 147 * 64; e += 256) {
        const int co = e / 147, tap = e - co * 147;   // (contiguous reads of the OIHW weights)
        ws[tap * 64 + co] = w[e];
    }
    if (tid < 64) cs[tid] = centre ? -centre[tid] : 0.f;
    for (int item = blockIdx.x; item < B * bands; item += gridDim.x) {
        const int b = item / bands, band = item - b * bands;
        const int oy0 = band * TH, iy0 = 2 * oy0 - 3;
        __syncthreads();                              // the previous item's readers are done (first item: weights visible)
        for (int e = tid; e < 3 * plane; e += 256) {
            const int c = e / plane, r = e - c * plane, ry = r / Wp, rx = r - ry * Wp;
            const int yin = iy0 + ry, xin = rx - 3;
            float v = 0.f;
            if ((unsigned)yin < (unsigned)Hin && (unsigned)xin < (unsigned)Win) v = x[(((long)b * 3 + c) * Hin + yin) * Win + xin];
            xs[e] = v;
        }
        __syncthreads();
        const int n_out = min(TH, Ho - oy0) * Wo, nblk = (n_out + 63) / 64;
        for (int u = wave; u < 4 * nblk; u += 4) {
            const int chunk = u / nblk, blk = u - chunk * nblk;
            const int q = blk * 64 + lane;
            const bool ok = q < n_out;
            const int qq = ok ? q : 0, ty = qq / Wo, ox = qq - ty * Wo;
            float acc[16];
#pragma unroll
            for (int o = 0; o < 16; ++o) acc[o] = cs[chunk * 16 + o];
            const float* xb = xs + (2 * ty) * Wp + 2 * ox;
            const float* wb = ws + chunk * 16;
            for (int c = 0; c < 3; ++c)
                for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const float xv = xb[c * plane + ky * Wp + kx];
                        const float* wt = wb + ((c * 7 + ky) * 7 + kx) * 64;
#pragma unroll
                        for (int o4 = 0; o4 < 4; ++o4) {
                            const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt + o4 * 4);
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[o4 * 4 + k] = fmaf(xv, w4[k], acc[o4 * 4 + k]);
                        }
                    }
                }
            if (ok) {
                float* dst = y + (((long)b * Ho + oy0 + ty) * Wo + ox) * 64 + chunk * 16;
#pragma unroll
                for (int o4 = 0; o4 < 4; ++o4)
                    *reinterpret_cast<f32x4*>(dst + o4 * 4) = f32x4{acc[o4 * 4], acc[o4 * 4 + 1], acc[o4 * 4 + 2], acc[o4 * 4 + 3]};
            }
        }
    }
}

}  // namespace

// ================================================================================================
// C ABI, and the pack launcher of cvcl_pack_conv_weight (csrc/resnext.hip; declared in cvcl_common.h)
// ================================================================================================
int cvcl_pack_stem_bf16(const float* w_oihw, void* out, void* stream) {
    hipLaunchKernelGGL(pack_stem_kernel, dim3(cvcl_div_up(4 * 6 * 512, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, (bf16_t*)out);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

static int stem_grid(int B, int Hin) {
    const int items = B * cvcl_div_up(Hin / 2, STEM_TH);
    return items < 512 ? items : 512;
}

extern "C" int cvcl_stem_conv_stats_rows(int dtype, int B, int H, int W) {
    if (!cvcl_dtype_trunk(dtype)) return 0;
    if (dtype == CVCL_F32X3) return cvcl_stem_split_stats_rows(B, H, W);
    if (dtype == CVCL_BF16) return stem_grid(B, H);
    return cvcl_col_stats_rows((long)B * (H / 2) * (W / 2));
}

extern "C" int cvcl_stem_conv7x7(int dtype, const float* x_nchw, const void* w_packed, void* y_nhwc, float* stats,
                                 int stats_rows, const float* centre, int B, int H, int W, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_stem_conv7x7");
    if (dtype == CVCL_F32X3)                           // split-bf16 products, statistics fused (csrc/conv_split.hip)
        return cvcl_stem_split(x_nchw, w_packed, (float*)y_nhwc, stats, stats_rows, centre, B, H, W, stream);
    CVCL_CHECK_ARG(x_nchw && w_packed && (y_nhwc || (dtype == CVCL_BF16 && stats)) && B > 0 && H % 2 == 0 && W % 2 == 0,
                   "cvcl_stem_conv7x7: bad args");                 // (bf16: y_nhwc NULL = statistics only)
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CVCL_BF16) {
        CVCL_CHECK_ARG(W + 6 + 8 <= 2 * STEM_PITCH && W % 4 == 0 && W / 4 <= 64,
                       "cvcl_stem_conv7x7: width %d not supported by the staged patch", W);
        const int g = stem_grid(B, H);
        CVCL_CHECK_ARG(!stats || stats_rows >= g, "cvcl_stem_conv7x7: stats_rows %d < %d", stats_rows, g);
        const size_t lds = (size_t)3 * STEM_ROWS * STEM_PITCH * 4 + 4 * 16 * STEM_OPITCH + 64 * 4;
        float* st = stats;
        CVCL_CHECK_ARG(st, "cvcl_stem_conv7x7: the bf16 kernel always emits statistics; pass a buffer");
        CvclProfScope prof(stream, CVCL_K_STEM);
        hipLaunchKernelGGL(stem_mfma_kernel, dim3(g), dim3(256), lds, s, x_nchw, (const bf16_t*)w_packed, (bf16_t*)y_nhwc,
                           st, centre, B, H, W);
        CVCL_LAUNCH_CHECK();
        return CVCL_OK;
    }
    const long total = (long)B * (H / 2) * (W / 2) * 64;
    {
        CvclProfScope prof(stream, CVCL_K_STEM);
        // LDS-tiled kernel when a band of >= 1 output row fits (weights 37 KB + 3 x (2 TH + 5) x (W + 6) floats)
        const int Ho = H / 2;
        auto lds_of = [&](int th) { return (size_t)(147 * 64 + 64 + 3 * (2 * th + 5) * (W + 6)) * 4; };
        int TH = Ho < 8 ? Ho : 8;
        while (TH > 1 && lds_of(TH) > 150 * 1024) --TH;
        if (lds_of(TH) <= 150 * 1024) {
            static CvclLdsAttr attr;
            if (const int rc = cvcl_raise_lds_limit(attr, (const void*)stem_tiled_f32_kernel, 160 * 1024, "cvcl_stem_conv7x7")) return rc;
            attr.mark();
            const int bands = cvcl_div_up(Ho, TH);
            const long items = (long)B * bands;
            hipLaunchKernelGGL(stem_tiled_f32_kernel, dim3((unsigned)(items < 1024 ? items : 1024)), dim3(256), lds_of(TH), s, x_nchw,
                               (const float*)w_packed, (float*)y_nhwc, centre, B, H, W, TH, bands);
        } else {
            hipLaunchKernelGGL(stem_direct_f32_kernel, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, s, x_nchw,
                               (const float*)w_packed, (float*)y_nhwc, centre, B, H, W);
        }
    }
    CVCL_LAUNCH_CHECK();
    if (stats) return cvcl_col_stats(CVCL_F32, y_nhwc, (long)B * (H / 2) * (W / 2), 64, stats, stats_rows, stream);
    return CVCL_OK;
}

// conv1 7x7/2 + bn1 + relu + maxpool 3x3/2 in one pass (stem_pool_mfma_kernel; bf16): x NCHW fp32 -> y NHWC bf16 [B, H/4, W/4, 64]
extern "C" int cvcl_stem_pool_supported(int dtype, int H, int W) {
    return dtype == CVCL_BF16 && H % 2 == 0 && W % 4 == 0 && W / 4 <= 64 && W + 6 + 8 <= 2 * STEM_PITCH && W / 2 + 2 <= STEMP_BW;
}

extern "C" int cvcl_stem_pool(int dtype, const float* x_nchw, const void* w_packed, const float* scale, const float* shift,
                              const float* centre, void* y_nhwc, int B, int H, int W, void* stream) {
    CVCL_CHECK_DTYPE(dtype, "cvcl_stem_pool");
    CVCL_CHECK_ARG(x_nchw && w_packed && scale && shift && y_nhwc && B > 0, "cvcl_stem_pool: bad args");
    CVCL_CHECK_ARG(cvcl_stem_pool_supported(dtype, H, W), "cvcl_stem_pool: bf16 and a width <= %d only (got dtype %d, %d x %d)",
                   2 * (STEMP_BW - 2), dtype, H, W);
    const size_t lds = (size_t)3 * STEMP_ROWS * STEM_PITCH * 4 + (size_t)STEMP_BAND_BYTES + 3 * 64 * 4;
    static CvclLdsAttr attr;
    if (const int rc = cvcl_raise_lds_limit(attr, (const void*)stem_pool_mfma_kernel, (int)lds, "cvcl_stem_pool")) return rc;
    attr.mark();
    const int Hp = (H / 2 - 1) / 2 + 1;
    const int items = B * cvcl_div_up(Hp, STEMP_TP);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const int grid = items < cus ? items : cus;
    CvclProfScope prof(stream, CVCL_K_STEM);
    hipLaunchKernelGGL(stem_pool_mfma_kernel, dim3(grid), dim3(512), lds, (hipStream_t)stream, x_nchw, (const bf16_t*)w_packed,
                       (bf16_t*)y_nhwc, scale, shift, centre, B, H, W);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
