// The evaluation-time frame transform on the device (reference: multimodal_lit.py:143-147 -- Resize((224, 224), BICUBIC) -> ToTensor ->
// Normalize, the `preprocess` that load_model returns; the same transform in analysis_cvcl/alignment.py, embeddings.py:32-37,
// generate_attention_maps.py:63-67 and object_categories_data_module.py:49-52, 106-109; and CLIP's Resize(224, BICUBIC) ->
// CenterCrop(224) -> ToTensor -> Normalize, multimodal_data_module.py:259-266, object_categories_data_module.py:38-45).  The reference
// runs it per image on PIL images; here ONE launch transforms a ragged batch of decoded uint8 frames, bit-identically to Pillow's
// integer pixel arithmetic (tests/preprocess_common.py restates it, tests/golden/preprocess_pil.npz pins it against Pillow itself):
//
//   bicubic resize   Pillow Resample.c: separable Keys cubic (a = -0.5, support 2) widened by the down-scale factor; coefficients
//                    normalised in double, rounded to 22 fractional bits (-0.5 for negative weights); horizontal pass, then vertical
//                    pass, each started at 1 << 21, shifted right by 22 and clamped to uint8; a pass whose size does not change is
//                    the identity
//   centre crop      only the out_h x out_w window (origin ct, cl) of the rh x rw resized image is computed: output pixels are
//                    independent, so this is resize-then-crop bit for bit, and the crop costs nothing
//   ToTensor / Normalize   (u8 / 255 - mean) / std in fp32 (true divisions, as torch), written NCHW
//
// A source frame does not fit LDS the way augment.hip's 224 x 224 crop does, so a workgroup takes one frame and one BAND of output
// rows: it resamples horizontally the source rows that band's vertical taps reach (all three interleaved channels together: every
// source byte is read once per band, not once per plane) into an LDS tile [rows][out_w][3], then runs the vertical pass from LDS.
// The host picks the band height, one per launch: the tallest of 32, 16, ... 1 rows whose tile and coefficient tables fit 160 KB for
// the frame of the batch that needs most (4096 x 4096 -> 224 x 224: 75 taps per output index, 4 rows per band).
#include <algorithm>
#include <cmath>

#include "cvcl_common.h"

namespace {

constexpr int PRE_PB = 22;                 // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int PRE_THREADS = 512;
constexpr int PRE_MAX_BAND = 32;
constexpr int PRE_MAX_SRC = 4096;          // source height / width
constexpr int PRE_MAX_RESIZED = 65536;     // resized height / width (a 4096 x 256 source at shorter side 224 is 3584 wide)
constexpr int PRE_MAX_OUT = 1024;          // window height / width
constexpr size_t PRE_LDS = 160 * 1024;

struct PreDev {
    const unsigned char* frames;           // the packed frames
    const long long* table;                // [B][CVCL_PREPROCESS_TABLE_COLS], device copy
    float* out;                            // [B][3][OH][OW]
    unsigned char* out_u8;                 // optional [B][OH][OW][3]
    int OH, OW;
    int band;                              // output rows per workgroup
    int tile_rows;                         // rows of the LDS tile (>= the source rows any band of any frame reaches)
    int kmax_h, kmax_v;                    // coefficient slots per output index of the horizontal / vertical pass
    float mean[3], stdv[3];
};

// Pillow's bicubic_filter (a = -0.5)
#pragma clang fp contract(off)
__device__ inline double bicubic_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
    return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for output index xx (bicubic): bounds and integer taps into kk[0..kmax).
// in_size == out_size: the pass Pillow skips, as the one-tap identity
#pragma clang fp contract(off)
__device__ inline void bicubic_taps(int in_size, int out_size, int xx, int kmax, int* bounds, int* kk) {
    if (in_size == out_size) {
        bounds[0] = xx;
        bounds[1] = 1;
        for (int x = 0; x < kmax; ++x) kk[x] = x == 0 ? 1 << PRE_PB : 0;
        return;
    }
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > kmax) xmax = kmax;                                  // (never: kmax is Pillow's ksize; keeps the table writes inside)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < kmax; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = bicubic_filter((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
        }
        kk[x] = (int)(w * (double)(1 << PRE_PB) + (w < 0.0 ? -0.5 : 0.5));
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

__device__ inline unsigned char clip8(int ss) {
    ss >>= PRE_PB;
    return (unsigned char)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
}

__global__ __launch_bounds__(PRE_THREADS) void preprocess_frames_kernel(PreDev p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.y, y0 = blockIdx.x * p.band;
    const int OH = p.OH, OW = p.OW, roww = OW * 3;
    const int nrows = min(p.band, OH - y0);                        // output rows of this band
    const long long* t = p.table + (size_t)b * CVCL_PREPROCESS_TABLE_COLS;
    const int H = (int)t[1], W = (int)t[2], rh = (int)t[3], rw = (int)t[4], ct = (int)t[5], cl = (int)t[6];
    int* kH = (int*)smem;                                          // [OW][kmax_h] taps
    int* bH = kH + OW * p.kmax_h;                                  // [OW][2] first tap, tap count
    int* kV = bH + OW * 2;                                         // [band][kmax_v]
    int* bV = kV + p.band * p.kmax_v;                              // [band][2]
    unsigned char* T = (unsigned char*)(bV + p.band * 2);          // [tile_rows][OW][3]: the horizontally resampled source rows

    for (int i = threadIdx.x; i < OW + nrows; i += blockDim.x) {
        if (i < OW) bicubic_taps(W, rw, cl + i, p.kmax_h, bH + i * 2, kH + i * p.kmax_h);
        else bicubic_taps(H, rh, ct + y0 + (i - OW), p.kmax_v, bV + (i - OW) * 2, kV + (i - OW) * p.kmax_v);
    }
    __syncthreads();

    // the source rows [r0, r1) this band's vertical taps reach
    int r0 = bV[0], r1 = bV[0] + bV[1];
    for (int i = 1; i < nrows; ++i) {
        r0 = min(r0, bV[i * 2]);
        r1 = max(r1, bV[i * 2] + bV[i * 2 + 1]);
    }
    if (r1 - r0 > p.tile_rows) r1 = r0 + p.tile_rows;              // (never: the host sized the tile from the same bounds)

    // horizontal pass: source rows (global, HWC bytes) -> T[r1 - r0][OW][3]
    const unsigned char* src = p.frames + t[0];
    for (int idx = threadIdx.x; idx < (r1 - r0) * OW; idx += blockDim.x) {
        const int r = idx / OW, xx = idx - r * OW;
        const int n = bH[xx * 2 + 1];
        const unsigned char* row = src + ((size_t)(r0 + r) * W + bH[xx * 2]) * 3;
        const int* k = kH + xx * p.kmax_h;
        int s0 = 1 << (PRE_PB - 1), s1 = s0, s2 = s0;
        int x = 0;
        for (; x + 4 <= n; x += 4) {                               // 4 taps x 3 channels = 12 bytes as three (unaligned) dword loads
            unsigned w[3];
            __builtin_memcpy(w, row + x * 3, 12);
            const int k0 = k[x], k1 = k[x + 1], k2 = k[x + 2], k3 = k[x + 3];
            s0 += (int)(w[0] & 255) * k0 + (int)(w[0] >> 24) * k1 + (int)((w[1] >> 16) & 255) * k2 + (int)((w[2] >> 8) & 255) * k3;
            s1 += (int)((w[0] >> 8) & 255) * k0 + (int)(w[1] & 255) * k1 + (int)(w[1] >> 24) * k2 + (int)((w[2] >> 16) & 255) * k3;
            s2 += (int)((w[0] >> 16) & 255) * k0 + (int)((w[1] >> 8) & 255) * k1 + (int)(w[2] & 255) * k2 + (int)(w[2] >> 24) * k3;
        }
        for (; x < n; ++x) {                                       // the rest byte by byte: nothing is read past the last tap
            const int kx = k[x];
            s0 += (int)row[x * 3] * kx;
            s1 += (int)row[x * 3 + 1] * kx;
            s2 += (int)row[x * 3 + 2] * kx;
        }
        unsigned char* o = T + (size_t)r * roww + xx * 3;
        o[0] = clip8(s0);
        o[1] = clip8(s1);
        o[2] = clip8(s2);
    }
    __syncthreads();

    // vertical pass from LDS, then ToTensor + Normalize
    for (int idx = threadIdx.x; idx < nrows * roww; idx += blockDim.x) {
        const int i = idx / roww, j = idx - i * roww;
        const int ymin = bV[i * 2] - r0;
        int n = bV[i * 2 + 1];
        if (ymin + n > r1 - r0) n = r1 - r0 - ymin;                // (never, as above)
        const int* k = kV + i * p.kmax_v;
        const unsigned char* col = T + (size_t)ymin * roww + j;
        int ss = 1 << (PRE_PB - 1);
        for (int y = 0; y < n; ++y) ss += (int)col[(size_t)y * roww] * k[y];
        const unsigned char v = clip8(ss);
        const int x = j / 3, c = j - x * 3, y = y0 + i;
        p.out[(((size_t)b * 3 + c) * OH + y) * OW + x] = __fdiv_rn(__fdiv_rn((float)v, 255.0f) - p.mean[c], p.stdv[c]);
        if (p.out_u8) p.out_u8[((size_t)b * OH + y) * roww + j] = v;
    }
}

}  // namespace

// Pillow's ksize = ceil(support) * 2 + 1 for the bicubic filter (support 2, widened by a down-scale); 1 for the identity pass
static int pre_taps(int in_size, int out_size) {
    if (in_size == out_size) return 1;
    const double scale = (double)in_size / (double)out_size;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
// upper bound of the source rows that `band` consecutive output rows reach: last tap of the last row minus first tap of the first =
// floor(c_last + s + .5) - floor(c_first - s + .5) < (band - 1) scale + 2 s + 1
static int pre_band_rows(int in_size, int out_size, int band) {
    if (in_size == out_size) return band;
    const double scale = (double)in_size / (double)out_size;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    const double rows = (band - 1) * scale + 2.0 * support + 2.0;
    return rows < (double)in_size ? (int)rows : in_size;
}
static size_t pre_lds_bytes(int out_w, int band, int tile_rows, int kmax_h, int kmax_v) {
    return ((size_t)out_w * (kmax_h + 2) + (size_t)band * (kmax_v + 2)) * sizeof(int) + (size_t)tile_rows * out_w * 3;
}

// frames: the decoded uint8 RGB frames (HWC, each of its own size) packed into one device buffer of frames_bytes bytes.  table: HOST
// int64 [B][CVCL_PREPROCESS_TABLE_COLS] = byte offset, source H, W, resized rh, rw, window origin ct, cl; table_dev: the same table
// in device memory (the kernel reads that one; the host copy is what gets validated, before any launch).  mean / std3: 3 host floats
// each.  out: fp32 [B][3][out_h][out_w]; out_u8 (optional): the uint8 image before ToTensor.
extern "C" int cvcl_preprocess_frames(const void* frames, int64_t frames_bytes, const int64_t* table, const void* table_dev, int B,
                                      const float* mean, const float* std3, void* out, int out_h, int out_w, void* out_u8,
                                      void* stream) {
    CVCL_CHECK_ARG(frames && table && table_dev, "cvcl_preprocess_frames: null pointer (frames / table / table_dev)");
    CVCL_CHECK_ARG(mean && std3, "cvcl_preprocess_frames: null pointer (mean / std)");
    CVCL_CHECK_ARG(out, "cvcl_preprocess_frames: null pointer (out)");
    CVCL_CHECK_ARG(B > 0 && B <= 65535, "cvcl_preprocess_frames: B %d outside 1..65535", B);
    CVCL_CHECK_ARG(out_h >= 1 && out_h <= PRE_MAX_OUT && out_w >= 1 && out_w <= PRE_MAX_OUT,
                   "cvcl_preprocess_frames: output %d x %d outside 1..%d", out_h, out_w, PRE_MAX_OUT);
    int kmax_h = 1, kmax_v = 1;
    for (int b = 0; b < B; ++b) {
        const int64_t* t = table + (size_t)b * CVCL_PREPROCESS_TABLE_COLS;
        const int64_t off = t[0], H = t[1], W = t[2], rh = t[3], rw = t[4], ct = t[5], cl = t[6];
        CVCL_CHECK_ARG(H >= 1 && H <= PRE_MAX_SRC && W >= 1 && W <= PRE_MAX_SRC,
                       "cvcl_preprocess_frames: frame %d: source %lld x %lld outside 1..%d", b, (long long)H, (long long)W, PRE_MAX_SRC);
        CVCL_CHECK_ARG(rh >= 1 && rh <= PRE_MAX_RESIZED && rw >= 1 && rw <= PRE_MAX_RESIZED,
                       "cvcl_preprocess_frames: frame %d: resized %lld x %lld outside 1..%d", b, (long long)rh, (long long)rw,
                       PRE_MAX_RESIZED);
        CVCL_CHECK_ARG(ct >= 0 && cl >= 0 && ct + out_h <= rh && cl + out_w <= rw,
                       "cvcl_preprocess_frames: frame %d: the %d x %d window at (%lld, %lld) leaves the %lld x %lld resized image", b, out_h,
                       out_w, (long long)ct, (long long)cl, (long long)rh, (long long)rw);
        CVCL_CHECK_ARG(off >= 0 && off + H * W * 3 <= frames_bytes,
                       "cvcl_preprocess_frames: frame %d: bytes %lld..%lld outside the %lld-byte buffer", b, (long long)off,
                       (long long)(off + H * W * 3), (long long)frames_bytes);
        kmax_h = std::max(kmax_h, pre_taps((int)W, (int)rw));
        kmax_v = std::max(kmax_v, pre_taps((int)H, (int)rh));
    }
    // the tallest band whose tile fits for every frame
    int band = PRE_MAX_BAND, tile_rows = 0;
    for (;; band /= 2) {
        tile_rows = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t* t = table + (size_t)b * CVCL_PREPROCESS_TABLE_COLS;
            tile_rows = std::max(tile_rows, pre_band_rows((int)t[1], (int)t[3], band));
        }
        if (pre_lds_bytes(out_w, band, tile_rows, kmax_h, kmax_v) <= PRE_LDS || band == 1) break;
    }
    const size_t lds = pre_lds_bytes(out_w, band, tile_rows, kmax_h, kmax_v);
    CVCL_CHECK_ARG(lds <= PRE_LDS, "cvcl_preprocess_frames: a %d-tap filter at output width %d needs %zu bytes of LDS (limit %zu)",
                   std::max(kmax_h, kmax_v), out_w, lds, PRE_LDS);
    PreDev d;
    d.frames = (const unsigned char*)frames; d.table = (const long long*)table_dev;
    d.out = (float*)out; d.out_u8 = (unsigned char*)out_u8;
    d.OH = out_h; d.OW = out_w; d.band = band; d.tile_rows = tile_rows; d.kmax_h = kmax_h; d.kmax_v = kmax_v;
    for (int i = 0; i < 3; ++i) { d.mean[i] = mean[i]; d.stdv[i] = std3[i]; }
    static CvclLdsAttr attr_set;
    if (const int rc = cvcl_raise_lds_limit(attr_set, (const void*)preprocess_frames_kernel, (int)PRE_LDS, "cvcl_preprocess_frames")) return rc;
    attr_set.mark();
    hipLaunchKernelGGL(preprocess_frames_kernel, dim3(cvcl_div_up(out_h, band), B), dim3(PRE_THREADS), lds, (hipStream_t)stream, d);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
