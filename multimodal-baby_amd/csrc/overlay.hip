// Attention-map overlays (cvcl_hip.h "Attention overlays"): the last step of every attention-map path -- Grad-CAM pairs, per-word
// caption maps, the ViT's CLS attention and its rollouts -- as one batched device pass instead of the per-map host loop of
// getAttMap / preprocess_attn_map (multimodal/attention_maps.py): bicubic resize (cvcl_bicubic_resize), scipy's gaussian_filter
// (separable, mode "reflect"), min-max normalisation, colormap lookup, the x^gamma blend with the de-normalised frame, uint8.
//
// Kernels: blur_pass<0> (the filter along the rows axis), blur_pass<1> (along the columns, with one (min, max) partial per workgroup;
// with radius 0 and no store it is the min-max pass of blur = 0), overlay_kernel (partials combined in index order, normalise, colour,
// blend, store through the destination table).  The filter passes stage a tile with its halo in LDS; the weights are computed in double in the
// kernels' prologue (half of the symmetric kernel, in LDS).  No atomics: two calls give the same bits.
#include <math.h>

#include "cvcl_common.h"

namespace {

constexpr int OV_MAX_SIDE = 1024;                     // H, W
constexpr int OV_MAX_LUT = 1024;
constexpr int OV_MAXR = 82;                           // int(4 * 0.02 * 1024 + 0.5)
constexpr int OV_TX = 64, OV_TY = 32;                 // outputs of one filter workgroup: 32 rows x 64 columns, 4 waves x 8 rows
constexpr int OV_PX = 4;                              // pixels per thread of the last pass
constexpr int OV_ITERS = 4;                           // ... and 4-pixel groups per thread: a workgroup colours 4096 pixels per LUT load

// scipy.ndimage mode "reflect" (d c b a | a b c d | d c b a): the period-2n reflection, valid for any p
__device__ __forceinline__ int reflect_index(int p, int n) {
    int m = p % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// out[y][x] = sum_t w[|t - r|] in[..] along AXIS (0: rows, 1: columns) of one [H, W] map per tile triple.  PARTIALS: the
// workgroup's (min, max) over the outputs it owns -> part[(map * tiles + tile) * 2]; STORE: write the outputs.
template <int AXIS, bool PARTIALS, bool STORE>
__global__ __launch_bounds__(256) void blur_pass(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ part, int H,
                                                 int W, int r, double sigma, int tiles_x, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ double phi[OV_MAXR + 1];
    __shared__ float wl[OV_MAXR + 1];                 // wl[d]: the weight at distance d from the centre
    __shared__ float red[8];
    // scipy's kernel in double: exp(-t^2 / 2 sigma^2) over -r .. r, normalised to sum 1 (summed in index order by every thread alike)
    if ((int)threadIdx.x <= r) phi[threadIdx.x] = exp(-0.5 / (sigma * sigma) * (double)threadIdx.x * (double)threadIdx.x);
    __syncthreads();
    if ((int)threadIdx.x <= r) {
        double sum = 0.0;
        for (int d = -r; d <= r; ++d) sum += phi[d < 0 ? -d : d];
        wl[threadIdx.x] = (float)(phi[threadIdx.x] / sum);
    }
    const int map = blockIdx.x / tiles, t = blockIdx.x - map * tiles;
    const int y0 = (t / tiles_x) * OV_TY, x0 = (t % tiles_x) * OV_TX;
    const int LR = AXIS == 0 ? OV_TY + 2 * r : OV_TY, LC = AXIS == 1 ? OV_TX + 2 * r : OV_TX;
    const float* src = in + (long)map * H * W;
    for (int e = threadIdx.x; e < LR * LC; e += 256) {
        const int j = e / LC, i = e - j * LC;
        const int sy = AXIS == 0 ? reflect_index(y0 - r + j, H) : min(y0 + j, H - 1);
        const int sx = AXIS == 1 ? reflect_index(x0 - r + i, W) : min(x0 + i, W - 1);
        tile[e] = src[(long)sy * W + sx];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    float lo = INFINITY, hi = -INFINITY;
    for (int ty = wave; ty < OV_TY; ty += 4) {
        const int y = y0 + ty;
        const float* p = tile + ty * LC + lane;        // the first tap: r rows above (AXIS 0) or r columns left of (AXIS 1) the output
        const int step = AXIS == 0 ? LC : 1;
        float acc = 0.f;
        for (int k = 0; k <= 2 * r; ++k) acc = fmaf(wl[k < r ? r - k : k - r], p[k * step], acc);
        if (y < H && x < W) {
            if (STORE) out[((long)map * H + y) * W + x] = acc;
            lo = fminf(lo, acc);
            hi = fmaxf(hi, acc);
        }
    }
    if (PARTIALS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if (lane == 0) { red[wave] = lo; red[4 + wave] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float* d = part + ((long)map * tiles + t) * 2;
            d[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            d[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        }
    }
}

struct OvArgs {
    const float* x;                 // [M, H, W] maps at the output size (blurred when asked); unused with image_only
    const float* part; int tiles;   // (min, max) partials of x, `tiles` per map; unused with has_range / image_only
    const float* images; int N;
    const int32_t* image_of_map;
    const float* lut; int n_lut;
    const int64_t* dst_offset; long pitch, out_elems;
    float* out_f32; uint8_t* out_u8; float* out_map;
    int M, H, W;
    int has_range, image_only;
    float gamma, vmin, vmax;
    float mean[3], std[3];
};

__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)floorf(fminf(fmaxf(v, 0.f), 1.f) * 255.f + 0.5f); }

__global__ __launch_bounds__(256) void overlay_kernel(OvArgs a, int tiles_per_map) {
    __shared__ float lut[3 * OV_MAX_LUT];
    __shared__ float red[8];
    const int map = blockIdx.x / tiles_per_map, tile_i = blockIdx.x - map * tiles_per_map;
    const int H = a.H, W = a.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the map's range: the partials in index order (the same order on every workgroup of the map and in every call)
    float lo = a.vmin, hi = a.vmax;
    if (!a.image_only) {
        for (int i = threadIdx.x; i < 3 * a.n_lut; i += 256) lut[i] = a.lut[i];
        if (!a.has_range) {
            lo = INFINITY;
            hi = -INFINITY;
            const float* p = a.part + (long)map * a.tiles * 2;
            for (int i = threadIdx.x; i < a.tiles; i += 256) {
                lo = fminf(lo, p[2 * i]);
                hi = fmaxf(hi, p[2 * i + 1]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = fminf(lo, __shfl_xor(lo, o, 64));
                hi = fmaxf(hi, __shfl_xor(hi, o, 64));
            }
            if (lane == 0) { red[wave] = lo; red[4 + wave] = hi; }
            __syncthreads();
            lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        } else {
            __syncthreads();
        }
    }
    const float span = hi - lo;
    // where this map goes, and which frame lies under it; a map whose table entries point outside the buffers is left out
    const int img = a.image_of_map ? a.image_of_map[map] : map;
    const long off = a.dst_offset ? a.dst_offset[map] : (long)map * H * a.pitch;
    const bool img_ok = img >= 0 && img < a.N;
    const bool dst_ok = off >= 0 && off + (long)(H - 1) * a.pitch + 3L * W <= a.out_elems;
    if (!img_ok) return;
    const bool colour = (a.out_f32 || a.out_u8) && dst_ok;
    const int G = (W + OV_PX - 1) / OV_PX;
    const long groups = (long)H * G;
    const float* frame = a.images + (long)img * 3 * H * W;
    const bool vec_in = (W & 3) == 0;
    const bool vec_out = ((off | a.pitch) & 3) == 0 && vec_in;
    for (int it = 0; it < OV_ITERS; ++it) {
        const long g = ((long)tile_i * OV_ITERS + it) * 256 + threadIdx.x;
        if (g >= groups) break;
        const int y = (int)(g / G), x = (int)(g - (long)y * G) * OV_PX;
        const int n = min(OV_PX, W - x);
        const long pix = (long)y * W + x;
        float xs[OV_PX] = {0.f, 0.f, 0.f, 0.f}, ch[3][OV_PX];
        if (vec_in) {
            if (!a.image_only) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (long)map * H * W + pix);
#pragma unroll
                for (int q = 0; q < OV_PX; ++q) xs[q] = v[q];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(frame + (long)c * H * W + pix);
#pragma unroll
                for (int q = 0; q < OV_PX; ++q) ch[c][q] = v[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < OV_PX; ++q) {
                const long pq = pix + min(q, n - 1);
                if (!a.image_only) xs[q] = a.x[(long)map * H * W + pq];
#pragma unroll
                for (int c = 0; c < 3; ++c) ch[c][q] = frame[(long)c * H * W + pq];
            }
        }
        float o[OV_PX][3];
#pragma unroll
        for (int q = 0; q < OV_PX; ++q) {
            float v = 0.f, wgt = 0.f;
            int idx = 0;
            if (!a.image_only) {
                v = xs[q] - lo;
                if (span > 0.f) v = v / span;
                if (a.has_range) v = fminf(fmaxf(v, 0.f), 1.f);
                xs[q] = v;
                idx = min(max((int)(v * (float)a.n_lut), 0), a.n_lut - 1);
                wgt = powf(v, a.gamma);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float den = __fadd_rn(__fmul_rn(ch[c][q], a.std[c]), a.mean[c]);
                o[q][c] = a.image_only ? den : __fadd_rn(__fmul_rn(1.f - wgt, den), __fmul_rn(wgt, lut[3 * idx + c]));
            }
        }
        if (a.out_map && !a.image_only) {
            float* d = a.out_map + (long)map * H * W + pix;
            if (vec_in) {
                stream_store(f32x4{xs[0], xs[1], xs[2], xs[3]}, reinterpret_cast<f32x4*>(d));
            } else {
                for (int q = 0; q < n; ++q) d[q] = xs[q];
            }
        }
        if (!colour) continue;
        const long e = off + (long)y * a.pitch + 3L * x;
        if (a.out_f32) {
            float* d = a.out_f32 + e;
            if (vec_out) {
                stream_store(f32x4{o[0][0], o[0][1], o[0][2], o[1][0]}, reinterpret_cast<f32x4*>(d));
                stream_store(f32x4{o[1][1], o[1][2], o[2][0], o[2][1]}, reinterpret_cast<f32x4*>(d) + 1);
                stream_store(f32x4{o[2][2], o[3][0], o[3][1], o[3][2]}, reinterpret_cast<f32x4*>(d) + 2);
            } else {
                for (int q = 0; q < n; ++q)
                    for (int c = 0; c < 3; ++c) d[3 * q + c] = o[q][c];
            }
        }
        if (a.out_u8) {
            uint8_t* d = a.out_u8 + e;
            if (vec_out) {
                unsigned wds[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    unsigned u = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int f = 4 * k + b;
                        u |= (unsigned)to_u8(o[f / 3][f % 3]) << (8 * b);
                    }
                    wds[k] = u;
                }
                unsigned* dw = reinterpret_cast<unsigned*>(d);
                dw[0] = wds[0];
                dw[1] = wds[1];
                dw[2] = wds[2];
            } else {
                for (int q = 0; q < n; ++q)
                    for (int c = 0; c < 3; ++c) d[3 * q + c] = to_u8(o[q][c]);
            }
        }
    }
}

constexpr int kKnownFlags = CVCL_OVERLAY_BLUR | CVCL_OVERLAY_HAS_RANGE | CVCL_OVERLAY_IMAGE_ONLY;

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
inline bool sizes_ok(int M, int h, int w, int H, int W) {
    return M >= 1 && H >= 1 && W >= 1 && H <= OV_MAX_SIDE && W <= OV_MAX_SIDE && h >= 1 && w >= 1 && h <= H && w <= W;
}
inline int filter_tiles_x(int W) { return cvcl_div_up(W, OV_TX); }
inline int filter_tiles(int H, int W) { return filter_tiles_x(W) * cvcl_div_up(H, OV_TY); }
// full-size fp32 planes the call needs: the resized maps, and two more passes' worth when blurring
inline int planes(int h, int w, int H, int W, int flags) {
    if (flags & CVCL_OVERLAY_IMAGE_ONLY) return 0;
    const bool resize = h != H || w != W, blur = (flags & CVCL_OVERLAY_BLUR) != 0;
    return blur ? 2 : (resize ? 1 : 0);
}
inline size_t partial_bytes(int M, int H, int W, int flags) {
    if (flags & (CVCL_OVERLAY_IMAGE_ONLY | CVCL_OVERLAY_HAS_RANGE)) return 0;
    return round16((size_t)M * filter_tiles(H, W) * 2 * sizeof(float));
}

// scipy.ndimage.gaussian_filter(map, sigma) with sigma = 0.02 max(H, W) and truncate 4: the radius is int(4 sigma + 0.5)
inline double gaussian_sigma(int H, int W) { return 0.02 * (double)(H > W ? H : W); }
inline int gaussian_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

}  // namespace

extern "C" size_t cvcl_attn_overlay_workspace_bytes(int M, int h, int w, int H, int W, int flags) {
    if (!sizes_ok(M, h, w, H, W) || (flags & ~kKnownFlags)) return 0;
    return 16 + (size_t)planes(h, w, H, W, flags) * round16((size_t)M * H * W * sizeof(float)) + partial_bytes(M, H, W, flags);
}

extern "C" int cvcl_attn_overlay(const float* maps, int M, int h, int w, const float* images, int N, int H, int W, const float* mean,
                                 const float* std, const int32_t* image_of_map, const float* lut, int n_lut, int flags, float gamma,
                                 float vmin, float vmax, const int64_t* dst_offset, int64_t row_pitch, int64_t out_elems, float* out_f32,
                                 uint8_t* out_u8, float* out_map, void* workspace, size_t workspace_bytes, void* stream) {
    CVCL_CHECK_ARG(!(flags & ~kKnownFlags), "cvcl_attn_overlay: unknown flags 0x%x", flags);
    const bool image_only = (flags & CVCL_OVERLAY_IMAGE_ONLY) != 0, has_range = (flags & CVCL_OVERLAY_HAS_RANGE) != 0;
    const bool blur = (flags & CVCL_OVERLAY_BLUR) != 0 && !image_only;
    CVCL_CHECK_ARG(M >= 1 && N >= 1, "cvcl_attn_overlay: M %d maps and N %d images must be positive", M, N);
    CVCL_CHECK_ARG(H >= 1 && W >= 1 && H <= OV_MAX_SIDE && W <= OV_MAX_SIDE, "cvcl_attn_overlay: the output size %d x %d is outside 1 .. %d",
                   H, W, OV_MAX_SIDE);
    CVCL_CHECK_ARG(h >= 1 && w >= 1 && h <= H && w <= W, "cvcl_attn_overlay: the map size %d x %d is outside 1 x 1 .. %d x %d (H x W)", h, w, H, W);
    CVCL_CHECK_ARG(images && mean && std, "cvcl_attn_overlay: null images / mean / std");
    CVCL_CHECK_ARG(image_only || (maps && lut), "cvcl_attn_overlay: null maps / lut");
    CVCL_CHECK_ARG(image_only || (n_lut >= 2 && n_lut <= OV_MAX_LUT), "cvcl_attn_overlay: n_lut %d is outside 2 .. %d", n_lut, OV_MAX_LUT);
    CVCL_CHECK_ARG(image_only || (gamma >= 0.f && gamma <= 64.f), "cvcl_attn_overlay: gamma %g is outside 0 .. 64", (double)gamma);
    CVCL_CHECK_ARG(!has_range || image_only || (vmin == vmin && vmax == vmax), "cvcl_attn_overlay: vmin / vmax is NaN");
    CVCL_CHECK_ARG(out_f32 || out_u8 || (out_map && !image_only), "cvcl_attn_overlay: no output pointer");
    CVCL_CHECK_ARG(image_of_map || M <= N, "cvcl_attn_overlay: without image_of_map map m lies over image m, but M %d > N %d", M, N);
    if (out_f32 || out_u8) {
        CVCL_CHECK_ARG(row_pitch >= 3L * W, "cvcl_attn_overlay: row_pitch %ld is below 3 W = %d elements", (long)row_pitch, 3 * W);
        const int64_t need = dst_offset ? (int64_t)(H - 1) * row_pitch + 3L * W : (int64_t)M * H * row_pitch;
        CVCL_CHECK_ARG(out_elems >= need, "cvcl_attn_overlay: out_elems %ld cannot hold the output (%ld elements)", (long)out_elems, (long)need);
    }
    CVCL_CHECK_ARG(cvcl_aligned16(maps) && cvcl_aligned16(images) && cvcl_aligned16(out_f32) && cvcl_aligned16(out_u8) &&
                   cvcl_aligned16(out_map) && cvcl_aligned16(workspace), "cvcl_attn_overlay: maps / images / outputs / workspace must be 16-byte aligned");
    const size_t need_ws = cvcl_attn_overlay_workspace_bytes(M, h, w, H, W, flags);
    CVCL_CHECK_ARG(workspace && workspace_bytes >= need_ws, "cvcl_attn_overlay: workspace of %zu bytes, %zu needed", workspace_bytes, need_ws);
    const int ftiles = filter_tiles(H, W);
    const int G = cvcl_div_up(W, OV_PX);
    const int otiles = cvcl_div_up((long)H * G, 256L * OV_ITERS);
    CVCL_CHECK_ARG((long)M * ftiles <= 0x7fffffffL && (long)M * otiles <= 0x7fffffffL, "cvcl_attn_overlay: M = %d maps exceed the grid", M);

    const size_t plane = round16((size_t)M * H * W * sizeof(float));
    char* ws = (char*)workspace;
    float* buf0 = (float*)ws;
    float* buf1 = (float*)(ws + plane);
    float* part = (float*)(ws + (size_t)planes(h, w, H, W, flags) * plane);
    const float* x = maps;
    hipStream_t s = (hipStream_t)stream;
    if (!image_only && (h != H || w != W)) {
        const int rc = cvcl_bicubic_resize(maps, buf0, M, h, w, H, W, stream);
        if (rc != CVCL_OK) return rc;
        x = buf0;
    }
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const dim3 fgrid((unsigned)((long)M * ftiles));
    const int tx = filter_tiles_x(W);
    if (blur) {
        const double sigma = gaussian_sigma(H, W);
        const int r = gaussian_radius(sigma);
        const size_t lds0 = (size_t)(OV_TY + 2 * r) * OV_TX * sizeof(float), lds1 = (size_t)OV_TY * (OV_TX + 2 * r) * sizeof(float);
        hipLaunchKernelGGL((blur_pass<0, false, true>), fgrid, dim3(256), lds0, s, x, buf1, (float*)nullptr, H, W, r, sigma, tx, ftiles);
        CVCL_LAUNCH_CHECK();
        if (has_range)
            hipLaunchKernelGGL((blur_pass<1, false, true>), fgrid, dim3(256), lds1, s, (const float*)buf1, buf0, part, H, W, r, sigma, tx, ftiles);
        else
            hipLaunchKernelGGL((blur_pass<1, true, true>), fgrid, dim3(256), lds1, s, (const float*)buf1, buf0, part, H, W, r, sigma, tx, ftiles);
        CVCL_LAUNCH_CHECK();
        x = buf0;
    } else if (!image_only && !has_range) {
        hipLaunchKernelGGL((blur_pass<1, true, false>), fgrid, dim3(256), (size_t)OV_TY * OV_TX * sizeof(float), s, x, (float*)nullptr, part, H,
                           W, 0, 1.0, tx, ftiles);
        CVCL_LAUNCH_CHECK();
    }
    OvArgs a;
    a.x = x; a.part = part; a.tiles = ftiles;
    a.images = images; a.N = N; a.image_of_map = image_of_map;
    a.lut = lut; a.n_lut = n_lut;
    a.dst_offset = dst_offset; a.pitch = (out_f32 || out_u8) ? (long)row_pitch : 3L * W; a.out_elems = (long)out_elems;
    a.out_f32 = out_f32; a.out_u8 = out_u8; a.out_map = out_map;
    a.M = M; a.H = H; a.W = W;
    a.has_range = has_range; a.image_only = image_only;
    a.gamma = gamma; a.vmin = vmin; a.vmax = vmax;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
    hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)((long)M * otiles)), dim3(256), 0, s, a, otiles);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
