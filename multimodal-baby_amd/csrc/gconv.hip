// The grouped 3x3 convolution (32 groups, pad 1, stride 1 | 2) of the ResNeXt-50 Bottlenecks for gfx950 (reference: conv2 of
// torchvision.models.resnext50_32x4d's Bottleneck.forward with bn1 + relu ahead of it, reached at multimodal/multimodal.py:101
// through VisionEncoder.forward).  NHWC raw input, the producer's BatchNorm + ReLU applied on the load (a_scale / a_shift, or formed
// here from the producer's accumulators: finalize-on-load, csrc/bn.hip) -> NHWC raw output with its per-channel statistics.
//
//   gconv_mfma_kernel<WIDE, NPF, NMT>  bf16: MFMA 16x16x32 on 16-channel units (block-diagonal weights for 4/8 channels per group,
//                                      one tap x 32 channels per step for 32 per group; pack_gconv_kernel's layout), input band
//                                      staged in LDS with BN+ReLU applied on the way in; gconv_plan picks the band and the grid
//   gconv_tiled_f32_kernel<CG>, gconv_direct_f32_kernel
//                                      fp32 (parity mode): VALU kernels with identical semantics; statistics from cvcl_col_stats
// CVCL_F32X3 goes to csrc/conv_split.hip.
#include <type_traits>

#include "cvcl_common.h"

namespace {

// grouped 3x3: [C][cg][3][3] -> bf16 units of [KS][16 n][32 k]
//   cg <= 16: unit = 16-channel chunk, KS = 5, k = tapsel*16 + ci, tap = 2*ks + tapsel (tap 9 = zero),
//             block-diagonal: zero where input channel and output channel are in different groups
//   cg == 32: unit = (group, ntile), KS = 9 (= tap), k = ci
__global__ void pack_gconv_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int C, int cg) {
    const int KS = cg == 32 ? 9 : 5;
    const long total = (long)(C / 16) * KS * 512;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i & 31), n = (int)((i >> 5) & 15), ks = (int)((i >> 9) % KS), unit = (int)(i / ((long)KS * 512));
    const int co = unit * 16 + n;
    float v = 0.f;
    if (cg == 32) {
        v = w[((long)co * 32 + k) * 9 + ks];
    } else {
        const int tap = 2 * ks + (k >> 4), ci_abs = unit * 16 + (k & 15);
        if (tap < 9 && ci_abs / cg == co / cg) v = w[((long)co * cg + (ci_abs % cg)) * 9 + tap];
    }
    out[i] = (bf16_t)v;
}

// ------------------------------------------------------------------------------------------------
// grouped 3x3 convolution, pad 1, stride 1|2, NHWC raw in (BN+ReLU applied on load) -> NHWC raw out
// ------------------------------------------------------------------------------------------------
constexpr int GC_CS = 64;                  // channels per workgroup slab
constexpr int GC_PIXB = 144;               // LDS bytes per staged pixel (128 B of channels + pad; an odd number of 16-byte slots)

struct GconvDev {
    const void* x; const float* a_scale; const float* a_shift; const void* w; void* y; float* stats;
    const float* centre;            // storage centre of the output (NULL = 0): the accumulators start at -centre[channel]
    int B, H, W, C, cg, stride, Ho, Wo, TH, bands, rows_in;
    float act_floor; // 0 = ReLU after the affine; -inf = none (a_scale == NULL: plain convolution of x, used by the data gradient)
    BnSrc src;       // src.acc != NULL: the input's BatchNorm affine is formed here from its producer's accumulators (finalize-on-load)
    int stats_acc;   // stats is an int64 accumulator [8][2][C] (cvcl_common.h), not partial rows
};

template <bool WIDE, int NPF, int NMT>
__global__ __launch_bounds__(256, WIDE ? 2 : 3) void gconv_mfma_kernel(GconvDev p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bf16_t* __restrict__ x = (const bf16_t*)p.x;
    bf16_t* __restrict__ y = (bf16_t*)p.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pix = lane & 15, kb = lane >> 4;
    const int slab = blockIdx.y, c0 = slab * GC_CS;
    const int Wp = p.W + 2;                                       // staged row width incl. halo columns
    constexpr bool wide = WIDE;                                   // 32 channels per group (layer4) vs 4/8/16
    constexpr int KS = WIDE ? 9 : 5;
    // this wave's unit: 16 output channels [c0 + 16*wave, +16); for cg == 32 the unit's inputs are the
    // 32 channels of its group, else the same 16 channels (block-diagonal weights)
    const int unit = c0 / 16 + wave;
    const bf16_t* wu = (const bf16_t*)p.w + (long)unit * KS * 512;
    bf16x8 wf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(wu + (ks * 16 + pix) * 32 + kb * 8);
    const int in_ch_off = wide ? ((wave >> 1) * 32 + kb * 8) : (wave * 16 + (kb & 1) * 8);   // within the slab

    // staging role: 8 chunks (of 8 channels) per pixel, 32 pixels per pass
    const int s_chunk = tid & 7, s_pix0 = tid >> 3;
    f32x2 sc[4], sh[4];                                           // (channel pairs: the staging math runs on packed fp32)
    if (p.src.acc) {
        // finalize-on-load: this slab's 64 input channels from the producing convolution's accumulators (the band buffers are not
        // in use yet); the workgroups of grid column 0 publish the moments
        float* aff = reinterpret_cast<float*>(smem);
        bn_slice_affine<GC_CS>(p.src, c0, blockIdx.x == 0, aff, aff + 64);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cl = s_chunk * 8 + 2 * e;
            sc[e] = f32x2{aff[cl], aff[cl + 1]};
            sh[e] = f32x2{aff[64 + cl], aff[64 + cl + 1]};
        }
        __syncthreads();                                          // (the band staging below overwrites the scratch)
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ch = c0 + s_chunk * 8 + 2 * e;
            sc[e] = p.a_scale ? f32x2{p.a_scale[ch], p.a_scale[ch + 1]} : f32x2{1.f, 1.f};
            sh[e] = p.a_scale ? f32x2{p.a_shift[ch], p.a_shift[ch + 1]} : f32x2{0.f, 0.f};
        }
    }
    const bool relu_in = p.act_floor == 0.f;                      // (-inf: no activation -- the data-gradient use)
    f32x2 ssum[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, ssq[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};     // (channel pairs: packed fp32)

    const int npix_in = p.rows_in * Wp;
    const int n_out = p.TH * p.Wo, n_mt = cvcl_div_up(n_out, 16);
    // per-lane constants of the compute loop: LDS byte offset of each K step's tap (+ this lane's channel block),
    // first pixel's (row, column), output channel
    int tap_off[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        int tap = wide ? ks : 2 * ks + (kb >> 1);
        if (tap > 8) tap = 8;                                          // padded tap: its weights are zero
        const int ky = tap / 3, kx = tap - ky * 3;
        tap_off[ks] = (ky * Wp + kx) * GC_PIXB + in_ch_off * 2;
    }
    // the m-tiles (16 output pixels each) of a band are the same for every work item: per lane, the LDS byte offset of the tile's
    // first tap (< 64 KiB), its band row and whether it exists, packed offset | row << 16 | exists << 24 (NMT = 4 | 8 tiles:
    // gconv_plan keeps TH * Wo <= 128)
    int mtab[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) {
        const int q = pix + 16 * mt;
        const bool ok = mt < n_mt && q < n_out;
        const int ty = q / p.Wo, ox = q - ty * p.Wo;
        mtab[mt] = ok ? ((((ty * p.stride) * Wp + ox * p.stride) * GC_PIXB) | (ty << 16) | (1 << 24)) : 0;
    }
    char* s_out = smem + npix_in * GC_PIXB;                            // output band [TH * Wo pixels][GC_PIXB]
    // software pipeline over work items: the next band's pixels are loaded into registers (raw, no waiting) before
    // the current band is multiplied out of LDS; BN+ReLU and the LDS write happen one iteration later.
    // NPF = ceil(staged pixels / 32) rounded up to an even count (template parameter: every slot is loaded, see below)
    u32x4 pf[NPF];
    bool pf_in[NPF];
    // Every slot issues its load unconditionally from a clamped (always valid) address and the predicate only decides later whether
    // the value or the zero padding is staged.  With the loads inside divergent `if`s the compiler put an s_waitcnt vmcnt(0) in
    // front of each of them: ten serialized memory round trips per work item -- the kernel's phases simply added up (179 us for
    // layer 1, of which 86 were this chain).
    // (row, column) of this thread's staging slots inside the band are the same for every work item, so everything about a slot
    // that does not depend on the item is computed once (the kernel is bound by VALU issue): its band row, the element offset of
    // its (clamped) input column, and whether it is inside the band and not horizontal padding.  A slot that stages padding
    // still loads -- from the clamped neighbour pixel, a line the band reads anyway (a far-away dummy address showed up as +39 %
    // HBM reads in the PMC pass)
    int slot_y[NPF], slot_xoff[NPF];
    bool slot_ok[NPF];
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
        const int pi = s_pix0 + 32 * i;
        const int pc = min(pi, npix_in - 1);                          // (slots past the band re-read its last pixel)
        const int ry = pc / Wp, xin = pc - ry * Wp - 1;
        slot_y[i] = ry;
        slot_ok[i] = pi < npix_in && xin >= 0 && xin < p.W;
        slot_xoff[i] = min(max(xin, 0), p.W - 1) * p.C;
    }
    const int row_elems = p.W * p.C;
    auto prefetch = [&](int item) {
        const int b = item / p.bands, band = item - b * p.bands;
        const int iy0 = band * p.TH * p.stride - 1;
        const bf16_t* xb = x + (long)b * p.H * p.W * p.C + c0 + s_chunk * 8;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int yin = iy0 + slot_y[i];
            pf_in[i] = slot_ok[i] && (unsigned)yin < (unsigned)p.H;
            const int yc = min(max(yin, 0), p.H - 1);
            pf[i] = *reinterpret_cast<const u32x4*>(xb + (yc * row_elems + slot_xoff[i]));
        }
    };
    f32x4 acc_init = {0.f, 0.f, 0.f, 0.f};                             // output channel c0 + wave*16 + kb*4 + e
    if (p.centre) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(p.centre + c0 + wave * 16 + kb * 4);
        acc_init = f32x4{-cv[0], -cv[1], -cv[2], -cv[3]};
    }
    const int n_items = p.B * p.bands;
    const int st_off = (tid >> 3) * p.C + (tid & 7) * 8;             // store phase: this thread's chunk inside a band's output
    // the weight fragments (loaded above) are ready from here on: without this the compiler, conservative across the loop's back
    // edge, waits on vmcnt before the first MFMAs of every work item -- i.e. for the next item's prefetch just issued
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0) only
    // Work items in XCD-major order: block (x, y) has linear id x + y * gridDim.x and runs on XCD (linear id) % 8, every XCD with
    // an L2 of its own; consecutive items are adjacent bands of one image and share their halo rows.  With gridDim.x a multiple
    // of 8 the XCD is x % 8, and XCD j takes the contiguous item range [j * gridDim.x / 8, (j + 1) * gridDim.x / 8) of every round
    // (plain order: a band's neighbours sat on other XCDs and the halo rows were fetched twice: 2.12 GB read for 1.95 in the PMC pass)
    const int bx = (gridDim.x & 7) == 0 ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
    if (bx < n_items) prefetch(bx);
    for (int item = bx; item < n_items; item += gridDim.x) {
        const int b = item / p.bands, band = item - b * p.bands;
        const int oy0 = band * p.TH;
        __syncthreads();
        // staging without per-slot branches: every slot is transformed (relu(round(x * scale + shift)) on channel pairs:
        // v_pk_fma_f32, v_cvt_pk_bf16_f32, v_pk_max_i16), padding slots are then zeroed with a mask (zero padding lives in the
        // post-activation domain), and only the write itself is predicated (the last slot may lie past the band)
        auto stage = [&](auto RELU) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const int pi = s_pix0 + 32 * i;
                const unsigned keep = pf_in[i] ? 0xffffffffu : 0u;
                u32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned y = round2(__builtin_elementwise_fma(widen2(pf[i][e]), sc[e], sh[e]));
                    if constexpr (decltype(RELU)::value) y = relu2(y);
                    v[e] = y & keep;
                }
                if (pi < npix_in) *reinterpret_cast<u32x4*>(smem + pi * GC_PIXB + s_chunk * 16) = v;
            }
        };
        if (relu_in) stage(std::true_type{});
        else stage(std::false_type{});
        __syncthreads();
        if (item + (int)gridDim.x < n_items) prefetch(item + gridDim.x);
        // two independent m-tiles in flight per wave: their LDS reads and MFMA chains interleave
        const int rows_left = p.Ho - oy0;                            // (a last band may be partial)
#pragma unroll
        for (int mt = 0; mt < NMT; mt += 2) {
            if (mt >= n_mt) break;
            const int e0 = mtab[mt], e1 = mtab[mt + 1];
            const int base0 = e0 & 0xffff, base1 = e1 & 0xffff;
            const int q0 = pix + 16 * mt, q1 = q0 + 16;
            const bool wr0 = (e0 >> 24) && ((e0 >> 16) & 0xff) < rows_left, wr1 = (e1 >> 24) && ((e1 >> 16) & 0xff) < rows_left;
            f32x4 acc0 = acc_init, acc1 = acc_init;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(smem + base0 + tap_off[ks]);
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(smem + base1 + tap_off[ks]);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], a0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], a1, acc1, 0, 0, 0);
            }
            if (wr0) {
                const u32x2 o = {round2(f32x2{acc0[0], acc0[1]}), round2(f32x2{acc0[2], acc0[3]})};
                *reinterpret_cast<u32x2*>(s_out + q0 * GC_PIXB + wave * 32 + kb * 8) = o;
#pragma unroll
                for (int e = 0; e < 2; ++e) { const f32x2 sv = widen2(o[e]); ssum[e] += sv; ssq[e] = __builtin_elementwise_fma(sv, sv, ssq[e]); }
            }
            if (wr1) {
                const u32x2 o = {round2(f32x2{acc1[0], acc1[1]}), round2(f32x2{acc1[2], acc1[3]})};
                *reinterpret_cast<u32x2*>(s_out + q1 * GC_PIXB + wave * 32 + kb * 8) = o;
#pragma unroll
                for (int e = 0; e < 2; ++e) { const f32x2 sv = widen2(o[e]); ssum[e] += sv; ssq[e] = __builtin_elementwise_fma(sv, sv, ssq[e]); }
            }
        }
        // the band's output sits in LDS as [pixel][64 channels]: write it out as full 128-byte pixel rows
        // (16 B per lane).  Scattered 8-byte stores straight from the MFMA layout cost more than the whole
        // load + compute phases together (ablation in DESIGN.md).
        __syncthreads();
        const int valid_rows = min(p.TH, p.Ho - oy0);
        const int n_chunks = valid_rows * p.Wo * 8;
        // chunk tid + 256 k of the band (pixel (tid >> 3) + 32 k, channels 8 (tid & 7) ..): the element offset inside the band's
        // output rows is item-invariant up to the stride 32 C per k; only the band's base pointer changes per item
        bf16_t* yb = y + ((long)b * p.Ho + oy0) * p.Wo * p.C + c0 + st_off;
        const char* so = s_out + (tid >> 3) * GC_PIXB + (tid & 7) * 16;
#pragma unroll
        for (int k = 0; k < NMT / 2; ++k) {                   // NMT * 16 pixels * 8 chunks / 256 threads
            if (tid + 256 * k < n_chunks)
                *reinterpret_cast<bf16x8*>(yb + (long)k * 32 * p.C) = *reinterpret_cast<const bf16x8*>(so + k * 32 * GC_PIXB);
        }
    }
    // per-channel partial sums: reduce over the 16 pixel lanes; channel = c0 + wave*16 + kb*4 + e
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s = ssum[e >> 1][e & 1], q = ssq[e >> 1][e & 1];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (pix == 0 && p.stats) {
            const int ch = c0 + wave * 16 + kb * 4 + e;
            cvcl_bn_stats_out(p.stats, p.stats_acc, blockIdx.x, p.C, ch, s, q);
        }
    }
}

// fp32 parity path: direct grouped convolution, weights in the reference OIHW layout [C][cg][3][3]
__global__ __launch_bounds__(256) void gconv_direct_f32_kernel(const float* __restrict__ x, const float* __restrict__ a_scale,
                                                               const float* __restrict__ a_shift, const float* __restrict__ w,
                                                               float* __restrict__ y, const float* __restrict__ centre,
                                                               int B, int H, int W, int C, int cg,
                                                               int stride, int Ho, int Wo, float act_floor) {
    const long total = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % C);
        const long pp = i / C;
        const int ox = (int)(pp % Wo), oy = (int)((pp / Wo) % Ho), b = (int)(pp / ((long)Wo * Ho));
        const int g0 = (co / cg) * cg;
        float acc = centre ? -centre[co] : 0.f;
        for (int ci = 0; ci < cg; ++ci) {
            const float sc = a_scale ? a_scale[g0 + ci] : 1.f, sh = a_scale ? a_shift[g0 + ci] : 0.f;
            for (int ky = 0; ky < 3; ++ky) {
                const int yin = oy * stride - 1 + ky;
                if (yin < 0 || yin >= H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int xin = ox * stride - 1 + kx;
                    if (xin < 0 || xin >= W) continue;
                    const float v = fmaxf(fmaf(x[(((long)b * H + yin) * W + xin) * C + g0 + ci], sc, sh), act_floor);
                    acc = fmaf(v, w[((long)co * cg + ci) * 9 + ky * 3 + kx], acc);
                }
            }
        }
        y[i] = acc;
    }
}

// fp32 parity path, LDS-tiled, for the trunk's shapes (C % 64 == 0, 4 | 8 | 16 | 32 channels per group; anything else and bands that
// do not fit take the direct kernel above): one workgroup = one band of TH output rows of one image x one 64-channel slab.  The
// band's input (producer BN + ReLU applied, zero padding after it) is staged channel-major in LDS, the slab's weights transposed to
// [group][tap][ci][co]; a wave takes (group, 64 output pixels) units: lane = pixel, CG accumulators, per (tap, ci) one LDS read of
// the input value and CG FMAs against wave-uniform weights (broadcast 16-byte LDS reads).  ~60x the direct kernel at B = 256.
template <int CG>
__global__ __launch_bounds__(256) void gconv_tiled_f32_kernel(const float* __restrict__ x, const float* __restrict__ a_scale,
                                                              const float* __restrict__ a_shift, const float* __restrict__ w,
                                                              float* __restrict__ y, const float* __restrict__ centre,
                                                              int B, int H, int W, int C, int stride, int Ho, int Wo, int TH,
                                                              int bands, int plane_p, float act_floor) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    constexpr int NG = 64 / CG;
    const int Wp = W + 2, rows_in = (TH - 1) * stride + 3, plane = rows_in * Wp;
    float* ws = smf;                                  // [NG][9][CG ci][CG co]
    float* cs = ws + 64 * 9 * CG;                     // [64]  -centre
    float* xs = cs + 64;                              // [64][plane_p]  (plane_p = plane padded to 1 mod 8: staging writes spread over banks)
    const int c0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < 64 * CG * 9; e += 256) {    // OIHW [C][CG][3][3], read contiguously
        const int co = e / (CG * 9), r = e - co * (CG * 9), ci = r / 9, tap = r - ci * 9;
        const int g = co / CG, o = co - g * CG;
        ws[((g * 9 + tap) * CG + ci) * CG + o] = w[(long)c0 * CG * 9 + e];
    }
    if (tid < 64) cs[tid] = centre ? -centre[c0 + tid] : 0.f;
    const int ch4 = tid & 15;                         // staging role: 4 channels of a pixel
    f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
    if (a_scale) {
        sc4 = *reinterpret_cast<const f32x4*>(a_scale + c0 + ch4 * 4);
        sh4 = *reinterpret_cast<const f32x4*>(a_shift + c0 + ch4 * 4);
    }
    for (int item = blockIdx.x; item < B * bands; item += gridDim.x) {
        const int b = item / bands, band = item - b * bands;
        const int oy0 = band * TH, iy0 = oy0 * stride - 1;
        __syncthreads();                              // the previous item's readers are done (first item: weights visible)
        for (int pix = tid >> 4; pix < plane; pix += 16) {
            const int ry = pix / Wp, rx = pix - ry * Wp;
            const int yin = iy0 + ry, xin = rx - 1;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};           // zero padding lives in the post-activation domain
            if ((unsigned)yin < (unsigned)H && (unsigned)xin < (unsigned)W) {
                v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + yin) * W + xin) * C + c0 + ch4 * 4);
                if (a_scale) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = fmaxf(fmaf(v[k], sc4[k], sh4[k]), act_floor);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) xs[(ch4 * 4 + k) * plane_p + pix] = v[k];
        }
        __syncthreads();
        const int n_out = min(TH, Ho - oy0) * Wo, nblk = (n_out + 63) / 64;
        for (int u = wave; u < NG * nblk; u += 4) {
            const int g = u / nblk, blk = u - g * nblk;
            const int q = blk * 64 + lane;
            const bool ok = q < n_out;
            const int qq = ok ? q : 0, ty = qq / Wo, ox = qq - ty * Wo;
            float acc[CG];
#pragma unroll
            for (int o = 0; o < CG; ++o) acc[o] = cs[g * CG + o];
            const float* xb = xs + (g * CG) * plane_p + (ty * stride) * Wp + ox * stride;
            const float* wb = ws + g * 9 * CG * CG;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll 4
                for (int ci = 0; ci < CG; ++ci) {
                    const float xv = xb[ci * plane_p + ky * Wp + kx];
                    const float* wt = wb + (tap * CG + ci) * CG;
#pragma unroll
                    for (int o4 = 0; o4 < CG / 4; ++o4) {
                        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt + o4 * 4);
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[o4 * 4 + k] = fmaf(xv, w4[k], acc[o4 * 4 + k]);
                    }
                }
            }
            if (ok) {
                float* dst = y + (((long)b * Ho + oy0 + ty) * Wo + ox) * C + c0 + g * CG;
#pragma unroll
                for (int o4 = 0; o4 < CG / 4; ++o4)
                    *reinterpret_cast<f32x4*>(dst + o4 * 4) = f32x4{acc[o4 * 4], acc[o4 * 4 + 1], acc[o4 * 4 + 2], acc[o4 * 4 + 3]};
            }
        }
    }
}

}  // namespace

// ================================================================================================
// C ABI, and what csrc/resnext.hip calls (declared in cvcl_common.h): the pack launcher of cvcl_pack_conv_weight, cvcl_gconv3x3_src
// ================================================================================================
int cvcl_pack_gconv_bf16(const float* w_oihw, void* out, int cout, int cin_per_group, void* stream) {
    const long total = (long)(cout / 16) * (cin_per_group == 32 ? 9 : 5) * 512;
    hipLaunchKernelGGL(pack_gconv_kernel, dim3(cvcl_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, (bf16_t*)out, cout,
                       cin_per_group);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

namespace {
struct GconvPlan { int TH, bands, rows_in, grid_x; size_t lds; };
GconvPlan gconv_plan(int B, int H, int W, int C, int stride) {
    GconvPlan g;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, Wp = W + 2;
    // output rows per work item: staged input band + output band within ~52 KiB (3 workgroups per CU) and the
    // input pixel count within the 10 x 32 register-prefetch slots of the kernel
    auto bytes = [&](int th) { return (size_t)(((th - 1) * stride + 3) * Wp + th * Wo) * GC_PIXB; };
    int TH = Ho;
    while (TH > 1 && (bytes(TH) > (size_t)52 * 1024 || ((TH - 1) * stride + 3) * Wp > 10 * 32 || TH * Wo > 128)) TH = (TH + 1) / 2;
    g.TH = TH;
    g.bands = cvcl_div_up(Ho, TH);
    g.rows_in = (TH - 1) * stride + 3;
    g.lds = bytes(TH);
    // persistent grid = what is co-resident (no second round of workgroups): LDS- and register-limited to 3 per CU.
    // (Round 2 built a pipelined form -- one 512-thread workgroup per CU, double-buffered input / output bands, one barrier per
    // band, the two wave halves running store / stage / load and MFMA in opposite order: correct on every test and SLOWER,
    // 1.47 vs 1.05 ms per step.  Three small workgroups per CU hide each other's phases better than one pipelined one; removed.)
    int per_cu = (int)((160 * 1024) / g.lds);
    const int reg_limit = (C / 32 == 32) ? 2 : 3;                     // launch bounds of the two kernel variants
    if (per_cu > reg_limit) per_cu = reg_limit;
    if (per_cu < 1) per_cu = 1;
    const int slabs = C / GC_CS;
    int gx = per_cu * 256 / slabs;
    if (gx < 1) gx = 1;
    const int items = B * g.bands;
    g.grid_x = items < gx ? items : gx;
    return g;
}
}  // namespace

extern "C" int cvcl_gconv3x3_stats_rows(int dtype, int B, int H, int W, int C, int stride) {
    if (!cvcl_dtype_trunk(dtype)) return 0;
    if (dtype == CVCL_F32X3) return C % 32 == 0 ? cvcl_gconv_split_stats_rows(B, H, W, C, stride) : 0;
    if (dtype == CVCL_BF16) return gconv_plan(B, H, W, C, stride).grid_x;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    return cvcl_col_stats_rows((long)B * Ho * Wo);
}

// src != NULL (bf16 only, internal: the trunk's launch sequence): the input's BatchNorm affine is formed inside the kernel from its
// producer's int64 accumulators (finalize-on-load) instead of being read from a_scale / a_shift
int cvcl_gconv3x3_src(int dtype, const void* x, const float* a_scale, const float* a_shift, const BnSrc* src, const void* w_packed,
                      void* y, float* stats, int stats_rows, const float* centre, int B, int H, int W, int C, int groups,
                      int stride, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_gconv3x3");
    CVCL_CHECK_ARG(x && w_packed && y && (!a_scale == !a_shift), "cvcl_gconv3x3: null pointer");
    CVCL_CHECK_ARG(!src || (dtype == CVCL_BF16 && src->acc && src->gamma && src->beta && src->C == C && src->count > 0 &&
                            (const void*)src->acc != (const void*)stats),
                   "cvcl_gconv3x3: finalize-on-load source");
    CVCL_CHECK_ARG(stats_rows != CVCL_STATS_ACCUMULATE || dtype == CVCL_BF16, "cvcl_gconv3x3: accumulators exist for bf16 only");
    const float act_floor = (a_scale || src) ? 0.f : -INFINITY;
    CVCL_CHECK_ARG(B > 0 && (stride == 1 || stride == 2) && groups > 0 && C % groups == 0, "cvcl_gconv3x3: bad shape");
    const int cg = C / groups;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CVCL_F32X3)                           // split-bf16 products, statistics fused (csrc/conv_split.hip)
        return cvcl_gconv_split((const float*)x, a_scale, a_shift, act_floor, w_packed, (float*)y, stats, stats_rows, centre, B, H, W, C,
                                cg, stride, stream);
    if (dtype == CVCL_BF16) {
        CVCL_CHECK_ARG((cg == 4 || cg == 8 || cg == 16 || cg == 32) && C % GC_CS == 0,
                       "cvcl_gconv3x3: unsupported channels-per-group %d (C=%d)", cg, C);
        const GconvPlan g = gconv_plan(B, H, W, C, stride);
        CVCL_CHECK_ARG(g.lds <= 160 * 1024 && g.rows_in * (W + 2) <= 10 * 32 && g.TH * ((W - 1) / stride + 1) <= 128,
                       "cvcl_gconv3x3: feature map too wide for one staged band (%zu B, %d pixels)", g.lds, g.rows_in * (W + 2));
        CVCL_CHECK_ARG(!stats || stats_rows == CVCL_STATS_ACCUMULATE || stats_rows >= g.grid_x, "cvcl_gconv3x3: stats_rows %d < %d", stats_rows, g.grid_x);
        GconvDev d;
        d.x = x; d.a_scale = a_scale; d.a_shift = a_shift; d.w = w_packed; d.y = y; d.stats = stats; d.centre = centre;
        d.B = B; d.H = H; d.W = W; d.C = C; d.cg = cg; d.stride = stride; d.Ho = Ho; d.Wo = Wo;
        d.TH = g.TH; d.bands = g.bands; d.rows_in = g.rows_in;
        d.act_floor = act_floor;
        d.src = BnSrc{};
        d.stats_acc = stats && stats_rows == CVCL_STATS_ACCUMULATE;
        if (src) {
            CVCL_CHECK_ARG(g.lds >= 2048, "cvcl_gconv3x3: band buffers smaller than the finalize-on-load scratch");
            d.src = *src;
        }
        CvclProfScope prof(stream, CVCL_K_GCONV);
        int rc;
        const int slots = cvcl_div_up(g.rows_in * (W + 2), 32);
        static CvclLdsAttr attr_set[2][2][11];                 // per instantiation (wide, short m-tile table, slots)
        auto launch = [&](auto kern) -> int {
            CvclLdsAttr& done = attr_set[cg == 32][g.TH * Wo <= 64][slots <= 4 ? 4 : slots <= 6 ? 6 : slots <= 8 ? 8 : 10];
            if (const int rc = cvcl_raise_lds_limit(done, (const void*)kern, 160 * 1024, "cvcl_gconv3x3")) return rc;
            done.mark();
            hipLaunchKernelGGL(kern, dim3(g.grid_x, C / GC_CS), dim3(256), g.lds, s, d);
            return CVCL_OK;
        };
        const bool few = g.TH * Wo <= 64;                    // <= 4 m-tiles per band: the short m-tile table
#define CVCL_GCONV_PICK(W_) \
        (slots <= 4 ? (few ? launch(gconv_mfma_kernel<W_, 4, 4>) : launch(gconv_mfma_kernel<W_, 4, 8>)) \
         : slots <= 6 ? (few ? launch(gconv_mfma_kernel<W_, 6, 4>) : launch(gconv_mfma_kernel<W_, 6, 8>)) \
         : slots <= 8 ? (few ? launch(gconv_mfma_kernel<W_, 8, 4>) : launch(gconv_mfma_kernel<W_, 8, 8>)) \
                      : (few ? launch(gconv_mfma_kernel<W_, 10, 4>) : launch(gconv_mfma_kernel<W_, 10, 8>)))
        rc = cg == 32 ? CVCL_GCONV_PICK(true) : CVCL_GCONV_PICK(false);
#undef CVCL_GCONV_PICK
        if (rc) return rc;
        CVCL_LAUNCH_CHECK();
        return CVCL_OK;
    }
    const long total = (long)B * Ho * Wo * C;
    {
        CvclProfScope prof(stream, CVCL_K_GCONV);
        // LDS-tiled kernel for the trunk's shapes when a band fits: weights 64 x 9 x cg floats + 64 channel planes of the band
        auto plane_p_of = [&](int th) { const int pl = ((th - 1) * stride + 3) * (W + 2); return pl + ((9 - (pl & 7)) & 7); };   // = 1 mod 8
        auto lds_of = [&](int th) { return (size_t)(64 * 9 * cg + 64 + 64 * plane_p_of(th)) * 4; };
        int TH = Ho;
        while (TH > 1 && lds_of(TH) > 150 * 1024) --TH;
        const bool tiled = C % 64 == 0 && (cg == 4 || cg == 8 || cg == 16 || cg == 32) && lds_of(TH) <= 150 * 1024 &&
                           ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)a_scale & 15) == 0 && ((uintptr_t)a_shift & 15) == 0;
        if (tiled) {
            const int bands = cvcl_div_up(Ho, TH);
            const long items = (long)B * bands;
            const int slabs = C / 64;
            long gx = 1024 / slabs;                          // ~4 workgroups per CU in total; each stages its weights once
            if (gx < 1) gx = 1;
            if (gx > items) gx = items;
            static CvclLdsAttr attr[4];
            auto launch = [&](auto kern, int slot) -> int {
                if (const int rc = cvcl_raise_lds_limit(attr[slot], (const void*)kern, 160 * 1024, "cvcl_gconv3x3")) return rc;
                attr[slot].mark();
                hipLaunchKernelGGL(kern, dim3((unsigned)gx, slabs), dim3(256), lds_of(TH), s, (const float*)x, a_scale, a_shift,
                                   (const float*)w_packed, (float*)y, centre, B, H, W, C, stride, Ho, Wo, TH, bands, plane_p_of(TH), act_floor);
                return CVCL_OK;
            };
            const int rc = cg == 4 ? launch(gconv_tiled_f32_kernel<4>, 0) : cg == 8 ? launch(gconv_tiled_f32_kernel<8>, 1)
                         : cg == 16 ? launch(gconv_tiled_f32_kernel<16>, 2) : launch(gconv_tiled_f32_kernel<32>, 3);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(gconv_direct_f32_kernel, dim3(cvcl_grid(total, 256, 8192)), dim3(256), 0, s, (const float*)x, a_scale,
                               a_shift, (const float*)w_packed, (float*)y, centre, B, H, W, C, cg, stride, Ho, Wo, act_floor);
        }
    }
    CVCL_LAUNCH_CHECK();
    if (stats) return cvcl_col_stats(CVCL_F32, y, (long)B * Ho * Wo, C, stats, stats_rows, stream);
    return CVCL_OK;
}

extern "C" int cvcl_gconv3x3(int dtype, const void* x, const float* a_scale, const float* a_shift, const void* w_packed,
                             void* y, float* stats, int stats_rows, const float* centre, int B, int H, int W, int C, int groups,
                             int stride, void* stream) {
    return cvcl_gconv3x3_src(dtype, x, a_scale, a_shift, nullptr, w_packed, y, stats, stats_rows, centre, B, H, W, C, groups, stride, stream);
}
