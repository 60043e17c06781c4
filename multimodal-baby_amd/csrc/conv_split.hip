// Split-bf16 convolutions of the CVCL_F32X3 ("32-split") trunk: the 7x7/2 stem and the grouped 3x3 (stride 1 / 2), fp32 in / fp32 out.
//
// Arithmetic as csrc/gemm_split.hip: each fp32 operand is a sum of bf16 parts and a product is formed from the part products of
// rank i + j <= NT / 3 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Both convolutions are implicit GEMMs over one 32-channel
// output slab: out[m][co] = sum_k A[m][k] W[co][k], m an output pixel,
//   grouped 3x3: k = (tap, ci) over the 32 input channels of the slab (9 taps x 2 steps of 16); the weight is block-diagonal inside
//                the slab (zero where ci and co lie in different groups; cg = 32 has no zeros);
//   stem:        k = ci 49 + ky 7 + kx over the 147 taps of the 3 input planes (10 steps of 16, zero-padded).
// The weight is split and laid out once, when it is packed: [P][slabs][steps][32 co][16 k] bf16, so a lane's B fragment is 16
// contiguous bytes.  The A fragment (8 consecutive k of one pixel) is gathered by its lane straight from the fp32 input, the
// producer's BatchNorm + ReLU (a_scale / a_shift, grouped conv) applied in fp32 BEFORE the split, padding taps zero.
// One wave owns 32 pixels x 32 channels; a 4-wave workgroup 128 pixels of one slab, persistent over pixel tiles.  A lane holds one
// output channel of 16 pixels, so the per-channel BatchNorm sums of the stored values stay in two registers and are written once per
// workgroup as a partial row (deterministic; no statistics pass over the output).
#include "cvcl_common.h"

namespace {

constexpr int CS_BM = 128;                       // output pixels per workgroup tile
constexpr int CS_CO = 32;                        // output channels per slab
constexpr int CS_STEP = CS_CO * 16;              // bf16 weight elements per (slab, step) and part
constexpr int KS_GCONV = 18, KS_STEM = 10;

template <int NT> constexpr int split_parts_of() {
    static_assert(NT == 3 || NT == 6, "3 or 6 split terms");
    return NT == 3 ? 2 : 3;
}

struct ConvSplitDev {
    const float* x; const float* a_scale; const float* a_shift; float act_floor;
    const bf16_t* w;                             // packed [P][slabs][KS][32][16]
    float* y; float* stats; const float* centre;
    int H, W, C, stride, Ho, Wo, Cout;           // grouped conv: x NHWC [B,H,W,C], y [B,Ho,Wo,C]; stem: x NCHW [B,3,H,W], y [B,Ho,Wo,64]
    long M, w_part;
    int tiles_m;
};

// parts of x (gemm_split.hip split_parts: the largest finite bf16 for a finite x beyond the bf16 range, zero remainders for inf / NaN)
template <int P>
__device__ __forceinline__ void split8(const float* v, bf16x8* frag) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = v[j];
        const bf16_t h0 = (bf16_t)x;
        const bool hfin = __builtin_isfinite((float)h0), xfin = __builtin_isfinite(x);
        const bf16_t hmax = __builtin_bit_cast(bf16_t, (unsigned short)(x < 0.f ? 0xFF7F : 0x7F7F));
        const bf16_t h = (!hfin && xfin) ? hmax : h0;
        frag[0][j] = h;
        float r = xfin ? x - (float)h : 0.f;
#pragma unroll
        for (int i = 1; i < P; ++i) {
            const bf16_t q = (bf16_t)r;
            frag[i][j] = q;
            r -= (float)q;
        }
    }
}

template <bool STEM>
__device__ __forceinline__ void gather_a(const ConvSplitDev& p, int ks, int b, int oy, int ox, int slab, int h, float* v) {
    if constexpr (STEM) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = ks * 16 + h * 8 + j;
            const int ci = k / 49, r = k - ci * 49, ky = r / 7, kx = r - ky * 7;
            const int iy = oy * 2 - 3 + ky, ix = ox * 2 - 3 + kx;
            v[j] = (k < 147 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? p.x[(((long)b * 3 + ci) * p.H + iy) * p.W + ix] : 0.f;
        }
    } else {
        const int tap = ks >> 1, dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        const int iy = oy * p.stride + dy, ix = ox * p.stride + dx;
        const int c0 = slab * CS_CO + (ks & 1) * 16 + h * 8;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
            const f32x4* src = reinterpret_cast<const f32x4*>(p.x + (((long)b * p.H + iy) * p.W + ix) * p.C + c0);
            const f32x4 u0 = src[0], u1 = src[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = u0[j]; v[4 + j] = u1[j]; }
            if (p.a_scale) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = fmaxf(fmaf(v[j], p.a_scale[c0 + j], p.a_shift[c0 + j]), p.act_floor);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;              // zero padding of the (activated) input
        }
    }
}

template <bool STEM, int NT>
__global__ __launch_bounds__(256) void conv_split_kernel(ConvSplitDev p) {
    constexpr int P = split_parts_of<NT>();
    constexpr int KS = STEM ? KS_STEM : KS_GCONV;
    __shared__ float red[4][2][CS_CO];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int slab = blockIdx.y, n = slab * CS_CO + r32;
    const bf16_t* wl = p.w + ((long)slab * KS * CS_CO + r32) * 16 + h * 8;
    const float cen = p.centre ? p.centre[n] : 0.f;
    const long hw = (long)p.Ho * p.Wo;
    float s_acc = 0.f, q_acc = 0.f;
    for (int tm = blockIdx.x; tm < p.tiles_m; tm += gridDim.x) {
        const long m0 = (long)tm * CS_BM + wave * 32;
        const long mg = min(m0 + r32, p.M - 1);                  // the pixel this lane gathers (rows past M: masked at the store)
        const int b = (int)(mg / hw), rem = (int)(mg - (long)b * hw), oy = rem / p.Wo, ox = rem - oy * p.Wo;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
            float v[8];
            gather_a<STEM>(p, ks, b, oy, ox, slab, h, v);
            bf16x8 fa[P], fw[P];
#pragma unroll
            for (int pt = 0; pt < P; ++pt) fw[pt] = *reinterpret_cast<const bf16x8*>(wl + pt * p.w_part + ks * CS_STEP);
            split8<P>(v, fa);
            if constexpr (NT == 6) {                              // smallest terms first
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2], fw[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fw[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fw[2], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fw[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fw[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fw[0], acc, 0, 0, 0);
        }
        // lane (r32, h): channel n of pixels m0 + (r & 3) + 8 (r >> 2) + 4 h; for a fixed r the 32 lanes of a half store 128 B of a row
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < p.M) {
                const float val = acc[r] - cen;
                p.y[m * p.Cout + n] = val;
                s_acc += val;
                q_acc = fmaf(val, val, q_acc);
            }
        }
    }
    if (!p.stats) return;
    s_acc += __shfl_xor(s_acc, 32, 64);
    q_acc += __shfl_xor(q_acc, 32, 64);
    if (h == 0) { red[wave][0][r32] = s_acc; red[wave][1][r32] = q_acc; }
    __syncthreads();
    if (tid < CS_CO) {
        const float s = ((red[0][0][tid] + red[1][0][tid]) + red[2][0][tid]) + red[3][0][tid];
        const float q = ((red[0][1][tid] + red[1][1][tid]) + red[2][1][tid]) + red[3][1][tid];
        cvcl_bn_stats_out(p.stats, 0, blockIdx.x, p.Cout, slab * CS_CO + tid, s, q);
    }
}

// packed weight [P][slabs][KS][32 co][16 k]: element e of part 0 is (slab, step, co, k16)
template <bool STEM, int P>
__global__ void pack_conv_split_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int cout, int cg, long n) {
    constexpr int KS = STEM ? KS_STEM : KS_GCONV;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int k16 = (int)(e & 15), co = (int)((e >> 4) & 31);
        const long t = e >> 9;
        const int ks = (int)(t % KS), slab = (int)(t / KS);
        const int cog = slab * CS_CO + co;
        float x = 0.f;
        if constexpr (STEM) {
            const int k = ks * 16 + k16;
            if (k < 147) x = w[(long)cog * 147 + k];
        } else {
            const int tap = ks >> 1, cig = slab * CS_CO + (ks & 1) * 16 + k16;
            if (cig / cg == cog / cg) x = w[((long)cog * cg + (cig - (cog / cg) * cg)) * 9 + tap];
        }
        bf16x8 prt[P];                                           // (split8 works on 8 values: use lane 0 of each part)
        float v[8] = {x, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        split8<P>(v, prt);
#pragma unroll
        for (int pt = 0; pt < P; ++pt) out[pt * n + e] = prt[pt][0];
    }
}

// NT = 3 instantiated as well, so that the 3-term form keeps compiling
template __global__ void conv_split_kernel<true, 3>(ConvSplitDev);
template __global__ void conv_split_kernel<false, 3>(ConvSplitDev);

int conv_split_grid(long M, int slabs) {
    static int cus = 0;
    if (!cus) {
        int dev = 0, c = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus = c;
    }
    const long tiles = (M + CS_BM - 1) / CS_BM;
    long g = cvcl_div_up(4L * cus, slabs);                   // what is co-resident: 4 workgroups per CU
    if (g > tiles) g = tiles;
    if (g > 1024) g = 1024;
    return g < 1 ? 1 : (int)g;
}

template <bool STEM>
int launch_conv_split(ConvSplitDev& d, long M, int slabs, int stats_rows, void* stream) {
    const int gx = conv_split_grid(M, slabs);
    CVCL_CHECK_ARG(!d.stats || (stats_rows != CVCL_STATS_ACCUMULATE && stats_rows >= gx),
                   "32-split convolution: stats_rows %d < %d (partial rows only)", stats_rows, gx);
    d.M = M;
    d.tiles_m = (int)((M + CS_BM - 1) / CS_BM);
    d.w_part = (long)slabs * (STEM ? KS_STEM : KS_GCONV) * CS_STEP;
    CvclProfScope prof(stream, STEM ? CVCL_K_STEM : CVCL_K_GCONV);
    hipLaunchKernelGGL((conv_split_kernel<STEM, kSplitTerms>), dim3(gx, slabs), dim3(256), 0, (hipStream_t)stream, d);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

}  // namespace

size_t cvcl_split_conv_bytes(int stem, int cout) {
    return (size_t)kSplitParts * (cout / CS_CO) * (stem ? KS_STEM : KS_GCONV) * CS_STEP * 2;
}

int cvcl_pack_split_conv(int stem, const float* w, void* out, int cout, int cg, void* stream) {
    CVCL_CHECK_ARG(w && out && cout > 0 && cout % CS_CO == 0, "cvcl_pack_conv_weight: bad args");
    if (!stem) CVCL_CHECK_ARG(cg == 4 || cg == 8 || cg == 16 || cg == 32, "cvcl_pack_conv_weight: unsupported grouped conv %d/%d", cout, cg);
    const long n = (long)(cout / CS_CO) * (stem ? KS_STEM : KS_GCONV) * CS_STEP;
    const long g = cvcl_div_up(n, 256);
    const dim3 grid((unsigned)(g < 4096 ? g : 4096));
    if (stem) hipLaunchKernelGGL((pack_conv_split_kernel<true, kSplitParts>), grid, dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)out, cout, cg, n);
    else hipLaunchKernelGGL((pack_conv_split_kernel<false, kSplitParts>), grid, dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)out, cout, cg, n);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

int cvcl_stem_split_stats_rows(int B, int H, int W) { return conv_split_grid((long)B * (H / 2) * (W / 2), 2); }
int cvcl_gconv_split_stats_rows(int B, int H, int W, int C, int stride) {
    return conv_split_grid((long)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1), C / CS_CO);
}

int cvcl_stem_split(const float* x, const void* w, float* y, float* stats, int stats_rows, const float* centre, int B, int H, int W,
                    void* stream) {
    CVCL_CHECK_ARG(x && w && y && B > 0 && H % 2 == 0 && W % 2 == 0, "cvcl_stem_conv7x7(CVCL_F32X3): bad args");
    ConvSplitDev d = {};
    d.x = x; d.w = (const bf16_t*)w; d.y = y; d.stats = stats; d.centre = centre;
    d.H = H; d.W = W; d.C = 3; d.stride = 2; d.Ho = H / 2; d.Wo = W / 2; d.Cout = 64;
    return launch_conv_split<true>(d, (long)B * d.Ho * d.Wo, 2, stats_rows, stream);
}

int cvcl_gconv_split(const float* x, const float* a_scale, const float* a_shift, float act_floor, const void* w, float* y, float* stats,
                     int stats_rows, const float* centre, int B, int H, int W, int C, int cg, int stride, void* stream) {
    CVCL_CHECK_ARG(x && w && y && C % CS_CO == 0 && (cg == 4 || cg == 8 || cg == 16 || cg == 32) && cvcl_aligned16(x),
                   "cvcl_gconv3x3(CVCL_F32X3): needs C %% 32 == 0, 4 / 8 / 16 / 32 channels per group and a 16-byte aligned input");
    ConvSplitDev d = {};
    d.x = x; d.a_scale = a_scale; d.a_shift = a_shift; d.act_floor = act_floor;
    d.w = (const bf16_t*)w; d.y = y; d.stats = stats; d.centre = centre;
    d.H = H; d.W = W; d.C = C; d.stride = stride; d.Ho = (H - 1) / stride + 1; d.Wo = (W - 1) / stride + 1; d.Cout = C;
    return launch_conv_split<false>(d, (long)B * d.Ho * d.Wo, C / CS_CO, stats_rows, stream);
}
