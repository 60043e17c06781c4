// The ResNeXt-50 32x4d image encoder as launch sequences for gfx950 (reference: torchvision.models.resnext50_32x4d reached at
// multimodal/multimodal.py:101 through VisionEncoder.forward; factory :155-158, utils.py:207-209).  Host code only, but for the
// weight cast: the trunk's layer tables and workspace layouts, one Bottleneck (bottleneck_fwd), the walk over the 16 blocks, and the
// cvcl_resnext50_* entries that enqueue a whole pass on the caller's stream.
//
// Activations are NHWC.  "raw" tensors are convolution outputs *before* BatchNorm: every convolution kernel also emits per-channel
// statistics of what it stored, and the *consumer* of the raw tensor applies scale/shift(+ReLU) while loading (csrc/bn.hip).  The
// kernels launched from here:
//   stem 7x7/2 (3->64)                      csrc/stem.hip           (CVCL_F32X3: csrc/conv_split.hip)
//   grouped 3x3 (32 groups)                 csrc/gconv.hip          (CVCL_F32X3: csrc/conv_split.hip)
//   1x1 convolutions                        cvcl_gemm (csrc/gemm.hip and the kernels it routes to), csrc/bn_gram.hip
//   BatchNorm, elementwise passes, pooling  csrc/bn.hip
// The internal launchers among them are declared in cvcl_common.h.
#include <array>
#include <type_traits>

#include "cvcl_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// weight packing (reference layout OIHW fp32 -> kernel layout)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void cast_kernel(const float* __restrict__ in, T* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = ElemTraits<T>::from_f(in[i]);
}

}  // namespace

extern "C" size_t cvcl_packed_weight_bytes(int dtype, int kind, int cout, int cin_per_group, int k) {
    if (!cvcl_dtype_trunk(dtype)) return 0;
    if (dtype == CVCL_F32X3) {                         // split parts: csrc/gemm_split.hip (dense), csrc/conv_split.hip (stem, grouped 3x3)
        if (kind == CVCL_PACK_DENSE) return cvcl_split_dense_bytes((long)cout * cin_per_group * k * k);
        if (kind == CVCL_PACK_STEM7) return cout == 64 && cin_per_group == 3 && k == 7 ? cvcl_split_conv_bytes(1, cout) : 0;
        if (kind == CVCL_PACK_GCONV3) return k == 3 && cout % 32 == 0 ? cvcl_split_conv_bytes(0, cout) : 0;
        return 0;
    }
    const size_t es = dtype == CVCL_BF16 ? 2 : 4;
    if (dtype == CVCL_F32 || kind == CVCL_PACK_DENSE) return (size_t)cout * cin_per_group * k * k * es;
    if (kind == CVCL_PACK_STEM7) return (size_t)4 * 6 * 512 * 2;
    if (kind == CVCL_PACK_GCONV3) return (size_t)(cout / 16) * (cin_per_group == 32 ? 9 : 5) * 512 * 2;
    return 0;
}

extern "C" int cvcl_pack_conv_weight(int dtype, int kind, const float* w_oihw, void* out, int cout, int cin_per_group,
                                     int k, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_pack_conv_weight");
    CVCL_CHECK_ARG(w_oihw && out && cout > 0 && cin_per_group > 0, "cvcl_pack_conv_weight: bad args");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)cout * cin_per_group * k * k;
    if (dtype == CVCL_F32X3) {
        if (kind == CVCL_PACK_DENSE) return cvcl_pack_split_dense(w_oihw, out, n, stream);     // [parts][cout][cin] bf16
        if (kind == CVCL_PACK_STEM7) {
            CVCL_CHECK_ARG(cout == 64 && cin_per_group == 3 && k == 7, "cvcl_pack_conv_weight: stem must be 64x3x7x7");
            return cvcl_pack_split_conv(1, w_oihw, out, cout, 3, stream);
        }
        if (kind == CVCL_PACK_GCONV3) {
            CVCL_CHECK_ARG(k == 3, "cvcl_pack_conv_weight: grouped conv must be 3x3");
            return cvcl_pack_split_conv(0, w_oihw, out, cout, cin_per_group, stream);
        }
        cvcl_set_error("cvcl_pack_conv_weight: unknown kind %d", kind);
        return CVCL_EINVAL;
    }
    if (dtype == CVCL_F32) {                       // parity mode keeps the reference layout
        hipLaunchKernelGGL(cast_kernel<float>, dim3(cvcl_grid(n, 256, 4096)), dim3(256), 0, s, w_oihw, (float*)out, n);
    } else if (kind == CVCL_PACK_DENSE) {
        hipLaunchKernelGGL(cast_kernel<bf16_t>, dim3(cvcl_grid(n, 256, 4096)), dim3(256), 0, s, w_oihw, (bf16_t*)out, n);
    } else if (kind == CVCL_PACK_STEM7) {
        CVCL_CHECK_ARG(cout == 64 && cin_per_group == 3 && k == 7, "cvcl_pack_conv_weight: stem must be 64x3x7x7");
        return cvcl_pack_stem_bf16(w_oihw, out, stream);                                       // csrc/stem.hip
    } else if (kind == CVCL_PACK_GCONV3) {
        CVCL_CHECK_ARG(k == 3 && (cin_per_group == 4 || cin_per_group == 8 || cin_per_group == 16 || cin_per_group == 32) &&
                           cout % 64 == 0, "cvcl_pack_conv_weight: unsupported grouped conv %d/%d", cout, cin_per_group);
        return cvcl_pack_gconv_bf16(w_oihw, out, cout, cin_per_group, stream);                 // csrc/gconv.hip
    } else {
        cvcl_set_error("cvcl_pack_conv_weight: unknown kind %d", kind);
        return CVCL_EINVAL;
    }
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

// ------------------------------------------------------------------------------------------------
// whole-network forward (one C call enqueues every kernel of the trunk on the caller's stream)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int kLayers[4] = {3, 4, 6, 3};                 // Bottlenecks of layer1 .. layer4 (kTrunkLayers, kMaxC, kAffStride: cvcl_common.h)
enum { kConv1, kConv2, kConv3, kDownsample };             // a Bottleneck's layers, in the order of `layers`
static_assert(sizeof(EvalAffineAll::C) == sizeof(int) * kTrunkLayers && sizeof(ApplyMomentsAll::C) == sizeof(int) * kTrunkLayers,
              "the one-launch layer tables hold the whole trunk");

// channels of layer j of a Bottleneck of the given stage: conv1 and conv2 the width (2 planes, 32x4d), conv3 and downsample 4 planes
constexpr int block_layer_c(int stage, int j) { return (64 << stage) * (j < kConv3 ? 2 : 4); }

// channels of the 53 layers, in the order of `layers`: the stem's 64, then each block's
constexpr std::array<int, kTrunkLayers> kTrunkC = [] {
    std::array<int, kTrunkLayers> c = {64};
    int l = 1;
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < kLayers[st]; ++b)
            for (int j = 0; j < (b == 0 ? 4 : 3); ++j) c[l++] = block_layer_c(st, j);
    return c;
}();

// the layer table of a one-launch kernel over the whole trunk (EvalAffineAll, ApplyMomentsAll)
template <class T>
T trunk_table(const cvcl_convbn_params* layers) {
    T t;
    for (int l = 0; l < kTrunkLayers; ++l) {
        const cvcl_convbn_params& p = layers[l];
        t.rm[l] = p.running_mean; t.rv[l] = p.running_var; t.C[l] = kTrunkC[l];
        if constexpr (std::is_same_v<T, EvalAffineAll>) { t.gamma[l] = p.gamma; t.beta[l] = p.beta; }
        else t.nbt[l] = p.num_batches_tracked;
    }
    return t;
}

// A workspace is a run of regions, each starting on a 256-byte boundary.  Each entry's layout below takes its regions in order
// from the shape: the *_workspace_bytes query returns `bytes` of the layout at address 0, and the entry uses the pointers of the
// layout at its workspace.
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Regions {
    uintptr_t base;
    size_t end = 0;
    template <class T> T* take(size_t bytes) { T* p = (T*)(base + end); end += al256(bytes); return p; }
};
constexpr size_t kStatsBytes = (size_t)kMaxStatsRows * 2 * kMaxC * 4;  // statistics rows [kMaxStatsRows][2][C] floats
constexpr size_t kAccBytes = kTrunkAccLayer * 8;                       // one layer's BatchNorm accumulators
inline size_t act_elems(int B, int H, int W) {
    // largest activation: stem output [B, H/2, W/2, 64] == layer1 tensors [B, H/4, W/4, 256]
    return (size_t)B * (H / 2) * (W / 2) * 64;
}

// cvcl_resnext50_fwd
struct TrunkLayout {
    char *buf[5], *gram;
    float *stats, *affine, *centres;
    long long* acc;
    size_t bytes;
    TrunkLayout(int dtype, int B, int H, int W, void* base = nullptr) {
        Regions r{(uintptr_t)base};
        for (char*& b : buf) b = r.take<char>(act_elems(B, H, W) * (dtype == CVCL_BF16 ? 2 : 4));
        stats = r.take<float>(kStatsBytes);
        affine = r.take<float>((size_t)kTrunkLayers * kAffStride * 4);
        centres = r.take<float>((size_t)kTrunkLayers * kMaxC * 4);      // eval mode without caller centres: the running means
        gram = r.take<char>(cvcl_conv1x1_gram_workspace_bytes(256));
        acc = r.take<long long>(kTrunkLayers * kAccBytes);
        bytes = r.end;
    }
};

// cvcl_resnext50_block_fwd: R1 (also R3), R2, RD, statistics rows, 4 affines, Gram workspace, 4 layers' accumulators
struct BlockLayout {
    char *R1, *R2, *RD, *gram;
    float *stats, *affine;
    long long* acc;
    size_t bytes;
    BlockLayout(int dtype, int B, int h, int w, int stage, void* base = nullptr) {
        // >= every intermediate of the block: [B, h, w, outc] (R1 is [B, h, w, outc / 2])
        const size_t act = (size_t)B * h * w * ((size_t)256 << stage) * (dtype == CVCL_BF16 ? 2 : 4);
        Regions r{(uintptr_t)base};
        R1 = r.take<char>(act); R2 = r.take<char>(act); RD = r.take<char>(act);
        stats = r.take<float>(kStatsBytes);
        affine = r.take<float>((size_t)4 * kAffStride * 4);
        gram = r.take<char>(cvcl_conv1x1_gram_workspace_bytes(256));
        acc = r.take<long long>(4 * kAccBytes);
        bytes = r.end;
    }
};
}  // namespace

extern "C" size_t cvcl_resnext50_workspace_bytes(int dtype, int B, int H, int W) {
    return cvcl_dtype_trunk(dtype) ? TrunkLayout(dtype, B, H, W).bytes : 0;
}

extern "C" size_t cvcl_resnext50_centres_floats(void) { return (size_t)kTrunkLayers * kMaxC; }

// ------------------------------------------------------------------------------------------------
// One Bottleneck (torchvision Bottleneck.forward: conv1-bn1-relu, conv2(grouped 3x3, stride)-bn2-relu, conv3-bn3,
// + identity / downsample, relu) as the launch sequence the whole-trunk call uses, and the walk over the trunk's 16 blocks.
// ------------------------------------------------------------------------------------------------
namespace {
struct PassCtx {
    int dtype, B, training;
    float momentum, eps;
    float* stats;                    // statistics rows, kMaxStatsRows of them
    void* gram_ws;                   // cvcl_conv1x1_gram workspace (K = 256)
    void* stream;
};

// The BatchNorm state of consecutive layers, layer 0 first: layer l's (scale, shift) at aff + l * kAffStride; its storage centre
// ("Centred storage" in cvcl_hip.h) at cen + l * kMaxC; the batch moments the deferred-statistics pass leaves at
// mom + l * kAffStride; its accumulators [8][2][2048] at acc + l * kTrunkAccLayer, zeroed for this pass.  cen, mom, acc may be
// NULL: plain storage, running statistics updated in place, no finalize-on-load.
struct BnLayers {
    const cvcl_convbn_params* L;
    float *aff, *mom;
    const float* cen;
    long long* acc;
    float* scale(int l) const { return aff + (size_t)l * kAffStride; }
    float* shift(int l) const { return scale(l) + kMaxC; }
    const float* centre(int l) const { return cen ? cen + (size_t)l * kMaxC : nullptr; }
    float* moments(int l) const { return mom ? mom + (size_t)l * kAffStride : nullptr; }
    long long* acc_of(int l) const { return acc ? acc + (size_t)l * kTrunkAccLayer : nullptr; }
    BnLayers from(int l) const { return {L + l, scale(l), moments(l), centre(l), acc_of(l)}; }
    // finalize-on-load (csrc/bn.hip "finalize-on-load"): layer l's convolution ACCUMULATES its statistics into acc_of(l) and
    // the consumer of its raw output forms the affine itself from this source -- no cvcl_bn_finalize launch for that layer
    BnSrc src(const PassCtx& c, int l, long count, int C) const {
        return {acc_of(l), C, (double)count, L[l].gamma, L[l].beta, centre(l), L[l].running_mean, L[l].running_var,
                L[l].num_batches_tracked, c.momentum, c.eps, moments(l), kMaxC, scale(l), shift(l)};
    }
    // otherwise layer l's statistics rows -> its affine and running statistics (or moments)
    int finalize(const PassCtx& c, int l, int rows, long count, int C) const {
        if (!c.training) return CVCL_OK;                  // eval mode: every layer's affine was produced up front
        return cvcl_bn_finalize_launch(c.stats, rows, count, L[l].gamma, L[l].beta, L[l].running_mean, L[l].running_var,
                                       L[l].num_batches_tracked, c.momentum, c.eps, scale(l), shift(l), C, moments(l), kMaxC, centre(l),
                                       c.stream);
    }
};

// a Bottleneck's shape; li = the index of its first layer in the trunk's `layers`
struct BlockGeom {
    int stage, first, li, width, outc, inplanes, stride;
    int h, w, ho, wo;                // input and output map
    long m_in, m_out;                // pixels of the batch in and out: the rows of the GEMMs
};
BlockGeom block_geom(int B, int stage, bool first, int h, int w, int li) {
    const int outc = block_layer_c(stage, kConv3), stride = (stage > 0 && first) ? 2 : 1;
    const int ho = h / stride, wo = w / stride;
    return {stage, first, li, block_layer_c(stage, kConv1), outc, first ? (stage == 0 ? 64 : outc / 2) : outc, stride,
            h, w, ho, wo, (long)B * h * w, (long)B * ho * wo};
}

// the GEMM of the block's 1x1 convolution j: conv1 and the downsample read the block input A, conv3 reads the conv2 output A;
// the downsample of a strided block gathers every stride-th pixel of its h x w input
cvcl_gemm_args conv1x1_args(const BlockGeom& g, const cvcl_convbn_params* L, int j, const void* A, void* C) {
    cvcl_gemm_args a = {};
    const int K = j == kConv3 ? g.width : g.inplanes, N = j == kConv1 ? g.width : g.outc;
    a.A = A; a.W = L[j].w; a.C = C;
    a.M = (int)(j == kConv1 ? g.m_in : g.m_out); a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N;
    if (j == kDownsample && g.stride > 1) {
        a.gather_ho = g.ho; a.gather_wo = g.wo; a.gather_hi = g.h; a.gather_wi = g.w; a.gather_stride = g.stride;
    }
    return a;
}

// a block's tensors: input X, output dst; R1, R2, R3, RD the outputs of conv1, conv2, conv3 and the downsample
template <class T> struct BlockBufs { T* X; T* dst; T* R1; T* R2; T* R3; T* RD; };

// The 16 Bottlenecks behind the stem, whose h x w output is in buf[0]: block(geometry, tensors) for each.  Block inputs and
// outputs alternate between buf[0] and buf[1] and the last block writes layer4_out; every block's scratch is R1 = R3 = buf[2]
// (conv2 has read R1 before conv3 writes R3), R2 = buf[3], RD = buf[4].  On return h x w is layer 4's map.
template <class T, class F>
int walk_blocks(int B, int& h, int& w, T* const* buf, T* layer4_out, F&& block) {
    T *X = buf[0], *out = buf[1];
    int li = 1;
    for (int stage = 0; stage < 4; ++stage)
        for (int bi = 0; bi < kLayers[stage]; ++bi) {
            const BlockGeom g = block_geom(B, stage, bi == 0, h, w, li);
            T* dst = (stage == 3 && bi == kLayers[3] - 1) ? layer4_out : out;
            if (int rc = block(g, BlockBufs<T>{X, dst, buf[2], buf[3], buf[2], buf[4]})) return rc;
            out = X; X = dst;
            li += bi == 0 ? 4 : 3;
            h = g.ho; w = g.wo;
        }
    return CVCL_OK;
}

// bn: the block's layers (kConv1 .. kDownsample) and their BatchNorm state
int bottleneck_fwd(const PassCtx& c, const BlockGeom& g, const BlockBufs<char>& io, const BnLayers& bn) {
    const int dtype = c.dtype, stage = g.stage, first = g.first, training = c.training;
    void* stream = c.stream;
    const cvcl_convbn_params* L = bn.L;
    int rc;
    static const bool fol_on = cvcl_env_on("CVCL_FINALIZE_ON_LOAD");               // (0: partial rows + a bn_finalize launch per layer)
    const bool use_acc = fol_on && bn.acc && training && dtype == CVCL_BF16;
    // Which forms this block takes (the explanations sit at the launches below):
    //  pro         conv3 applies BN2 + ReLU on its operand load: layers 1-2 in bf16 (width 128 | 256, the K of gemm_pro.hip)
    //  fused_tail  conv3's epilogue writes the block output: layers 1-2 in bf16, and every bf16 stage in eval mode
    // so in train mode fused_tail == pro, and in eval mode pro implies fused_tail.
    const bool pro = dtype == CVCL_BF16 && stage < 2;
    const bool fused_tail = dtype == CVCL_BF16 && (stage < 2 || !training);
    static const bool gemm_pro_on = cvcl_env_on("CVCL_GEMM_PRO");
    const bool ds_recompute = gemm_pro_on && pro && first && stage == 0;      // layer1.0: stride 1, a K = 64 block input
    auto gram_stats = [&](int l, const void* A, int K, const float* a_scale, const float* a_shift, int a_relu, const BnSrc* src = nullptr) -> int {
        const double* gram = nullptr;
        int r = cvcl_conv1x1_gram_src(A, K, g.m_out, K, src ? nullptr : a_scale, src ? nullptr : a_shift, src, a_relu, c.gram_ws,
                                      cvcl_conv1x1_gram_workspace_bytes(256), &gram, stream);
        if (r) return r;
        return cvcl_bn_from_gram(gram, K, g.m_out, L[l].w, K, g.outc, L[l].gamma, L[l].beta, L[l].running_mean, L[l].running_var,
                                 L[l].num_batches_tracked, c.momentum, c.eps, bn.scale(l), bn.shift(l), bn.moments(l), kMaxC,
                                 bn.centre(l), stream);
    };
    // The downsample branch of a stage's first block runs FIRST: its operand X was just written by the previous kernel and still
    // sits in the Infinity Cache (after conv1 / conv2 / conv3 it no longer does).
    // layer1.0 (bf16, fused tail, BN-prologue kernel): the branch is a K = 64 product of the block input, recomputed inside the tail
    // pass (gemm_pro.hip PRO_TAIL_DS) instead of being written to HBM (411 MB at B = 256) and read back; its own launch shrinks to a
    // Gram launch for its BN statistics (train mode) or disappears (eval mode).
    // BN2 of layers 1-2: formed by the Gram launch (the first reader of relu(bn2(.)); it publishes the affine for the tail pass behind
    // it).  (Layers 3-4 keep partial rows + cvcl_bn_finalize for BN2 / BN3 / the downsample BatchNorm: their consumers are elementwise
    // passes whose workgroups touch every channel.  Re-blocked into channel-sliced 1024-thread workgroups that finalize on load they
    // cost 2-3 us more per launch than the launch they save once two passes overlap: profiles/r06_fol_ab.txt.)
    const bool fol2 = use_acc && pro;
    if (first) {
        if (ds_recompute) {
            if (training && (rc = gram_stats(kDownsample, io.X, g.inplanes, nullptr, nullptr, 0))) return rc;
        } else {
            // downsample 1x1 stride s: X -> RD [m_out, outc]
            cvcl_gemm_args a = conv1x1_args(g, L, kDownsample, io.X, io.RD);
            a.stats = training ? c.stats : nullptr; a.stats_rows = kMaxStatsRows;
            a.centre = bn.centre(kDownsample);
            if ((rc = cvcl_gemm(dtype, &a, stream))) return rc;
            if ((rc = bn.finalize(c, kDownsample, a.stats ? cvcl_gemm_stats_rows(dtype, &a) : 0, g.m_out, g.outc))) return rc;
        }
    }
    // conv1 1x1: X [m_in, inplanes] -> R1 [m_in, width]
    int rows1 = 0;
    const bool fol1 = use_acc;
    {
        cvcl_gemm_args a = conv1x1_args(g, L, kConv1, io.X, io.R1);
        a.stats = training ? (fol1 ? (float*)bn.acc_of(kConv1) : c.stats) : nullptr;
        a.stats_rows = fol1 ? CVCL_STATS_ACCUMULATE : kMaxStatsRows;
        a.centre = bn.centre(kConv1);
        if ((rc = cvcl_gemm(dtype, &a, stream))) return rc;
        rows1 = training ? cvcl_gemm_stats_rows(dtype, &a) : 0;
    }
    // BN1's statistics -> affine: inside conv2's prologue (every workgroup of the grouped convolution normalises one fixed slab of
    // 64 channels: 16 accumulator loads per channel)
    if (!fol1 && (rc = bn.finalize(c, kConv1, rows1, g.m_in, g.width))) return rc;
    // conv2 grouped 3x3 (stride here): R1 -> R2 [m_out, width], BN1+ReLU fused into the load
    {
        const BnSrc src1 = fol1 ? bn.src(c, kConv1, g.m_in, g.width) : BnSrc{};
        if ((rc = cvcl_gconv3x3_src(dtype, io.R1, fol1 ? nullptr : bn.scale(kConv1), fol1 ? nullptr : bn.shift(kConv1), fol1 ? &src1 : nullptr,
                                    L[kConv2].w, io.R2, training ? (fol2 ? (float*)bn.acc_of(kConv2) : c.stats) : nullptr,
                                    fol2 ? CVCL_STATS_ACCUMULATE : kMaxStatsRows, bn.centre(kConv2), c.B, g.h, g.w, g.width, 32, g.stride,
                                    stream))) return rc;
    }
    if (!fol2 && (rc = bn.finalize(c, kConv2, training ? cvcl_gconv3x3_stats_rows(dtype, c.B, g.h, g.w, g.width, g.stride) : 0, g.m_out,
                                   g.width))) return rc;
    // conv3 1x1: relu(bn2(R2)) -> R3 [m_out, outc].  Layers 1-2 (K = width <= 256, bandwidth-bound): BN2 + ReLU rides conv3's
    // operand load (gemm_pro.hip: applied once per element, W resident in registers) -- no pass of its own over the tensor.
    // Layers 3-4 (MFMA-bound, 4-8 column-tile workgroups per A tile): BN2 + ReLU is applied in place first (one pass over the
    // narrow tensor), which is cheaper than repeating it in every column tile's operand path.
    if (!pro) {
        if ((rc = cvcl_bn_relu_apply(dtype, io.R2, bn.scale(kConv2), bn.shift(kConv2), io.R2, g.m_out, g.width, stream))) return rc;
    }
    // Layers 1-2 in bf16: conv3 is HBM-bound and cheap there, so it runs twice -- a statistics-only pass (reads only the narrow
    // operand), then a pass whose epilogue applies BN3 + identity / normalised downsample + ReLU and writes the block output --
    // instead of materialising raw3 and re-reading it in bn_add_relu (saves one write and one read of the wide tensor; results are
    // bit-identical).  Both passes apply BN2 + ReLU on the operand load (gemm_pro.hip).  Measured per step at B = 256 (round 2,
    // with gemm_pro): 1 stage 5.47 ms, 2 stages 5.46 ms and 1.2 GB less HBM traffic; layers 3-4 are MFMA-bound and keep the
    // materialised form.
    // In eval mode there is no statistics pass at all, so the fused tail is used in every stage.
    auto conv3_args = [&](void* C) {
        cvcl_gemm_args a = conv1x1_args(g, L, kConv3, io.R2, C);
        if (pro) { a.a_scale = bn.scale(kConv2); a.a_shift = bn.shift(kConv2); a.a_relu = 1; }
        a.centre = bn.centre(kConv3);
        return a;
    };
    // Train mode with the fused tail: BN3's batch statistics are needed before the product exists.  They come from the Gram matrix
    // of the operand (bn_gram.hip: sum y = w.s, sum y^2 = w^T G w -- one read of the narrow tensor, K <= 256 <= N / 2) instead of
    // a statistics-only run of the whole GEMM.  Without the fused tail, conv3 is materialised (with its statistics in train mode);
    // eval mode with the fused tail launches nothing here (the affine came from the running stats up front).
    if (fused_tail && training) {
        const BnSrc s2 = fol2 ? bn.src(c, kConv2, g.m_out, g.width) : BnSrc{};
        if ((rc = gram_stats(kConv3, io.R2, g.width, bn.scale(kConv2), bn.shift(kConv2), 1, fol2 ? &s2 : nullptr))) return rc;
    } else if (!fused_tail) {
        cvcl_gemm_args a = conv3_args(io.R3);
        a.stats = training ? c.stats : nullptr; a.stats_rows = kMaxStatsRows;
        if ((rc = cvcl_gemm(dtype, &a, stream))) return rc;
        if ((rc = bn.finalize(c, kConv3, a.stats ? cvcl_gemm_stats_rows(dtype, &a) : 0, g.m_out, g.outc))) return rc;
    }
    if (fused_tail) {
        cvcl_gemm_args a = conv3_args(io.dst);
        a.act = CVCL_ACT_RELU;
        a.c_scale = bn.scale(kConv3); a.c_shift = bn.shift(kConv3);
        if (ds_recompute) {
            a.A2 = io.X; a.W2 = L[kDownsample].w; a.K2 = g.inplanes; a.lda2 = g.inplanes; a.ldw2 = g.inplanes;
            a.centre2 = bn.centre(kDownsample);
        } else {
            a.R = first ? io.RD : io.X; a.ldr = g.outc;
        }
        if (first) { a.r_scale = bn.scale(kDownsample); a.r_shift = bn.shift(kDownsample); }
        if ((rc = cvcl_gemm(dtype, &a, stream))) return rc;
    } else if (first) {
        if ((rc = cvcl_bn_add_relu(dtype, io.R3, bn.scale(kConv3), bn.shift(kConv3), io.RD, bn.scale(kDownsample), bn.shift(kDownsample),
                                   io.dst, g.m_out, g.outc, stream))) return rc;
    } else {
        if ((rc = cvcl_bn_add_relu(dtype, io.R3, bn.scale(kConv3), bn.shift(kConv3), io.X, nullptr, nullptr, io.dst, g.m_out, g.outc,
                                   stream))) return rc;
    }
    return CVCL_OK;
}
}  // namespace

extern "C" size_t cvcl_resnext50_block_workspace_bytes(int dtype, int B, int h, int w, int stage) {
    return cvcl_dtype_trunk(dtype) ? BlockLayout(dtype, B, h, w, stage).bytes : 0;
}

extern "C" int cvcl_resnext50_block_fwd(int dtype, int B, int h, int w, int stage, int first, int training, const void* x_nhwc,
                                        const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                                        void* out_nhwc, float momentum, float eps, const float* centres, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_resnext50_block_fwd");
    CVCL_CHECK_ARG(x_nhwc && layers && workspace && out_nhwc, "cvcl_resnext50_block_fwd: null pointer");
    CVCL_CHECK_ARG(((uintptr_t)centres & 15) == 0, "cvcl_resnext50_block_fwd: centres must be 16-byte aligned");
    CVCL_CHECK_ARG(stage >= 0 && stage < 4 && n_layers == (first ? 4 : 3), "cvcl_resnext50_block_fwd: stage %d with %d layers", stage, n_layers);
    CVCL_CHECK_ARG(B > 0 && h > 0 && w > 0 && (!(stage > 0 && first) || (h % 2 == 0 && w % 2 == 0)), "cvcl_resnext50_block_fwd: bad shape");
    const BlockLayout ws(dtype, B, h, w, stage, workspace);
    if (workspace_bytes < ws.bytes) {
        cvcl_set_error("cvcl_resnext50_block_fwd: workspace too small");
        return CVCL_EWORKSPACE;
    }
    long long* acc = (training && dtype == CVCL_BF16) ? ws.acc : nullptr;
    if (acc && hipMemsetAsync(acc, 0, (size_t)n_layers * kAccBytes, (hipStream_t)stream) != hipSuccess) {
        cvcl_set_error("cvcl_resnext50_block_fwd: cannot clear the BatchNorm accumulators");
        return CVCL_ELAUNCH;
    }
    const BnLayers bn = {layers, ws.affine, nullptr, centres, acc};
    if (!training)                                        // eval mode: affines from the running statistics
        for (int l = 0; l < n_layers; ++l)
            if (int rc = cvcl_bn_eval_affine(layers[l].gamma, layers[l].beta, layers[l].running_mean, layers[l].running_var, eps,
                                             bn.scale(l), bn.shift(l), bn.centre(l), block_layer_c(stage, l), stream)) return rc;
    const PassCtx ctx = {dtype, B, training, momentum, eps, ws.stats, ws.gram, stream};
    return bottleneck_fwd(ctx, block_geom(B, stage, first != 0, h, w, 0),
                          BlockBufs<char>{(char*)x_nhwc, (char*)out_nhwc, ws.R1, ws.R2, ws.R1, ws.RD}, bn);
}

static int resnext50_fwd_impl(int dtype, int B, int H, int W, int training, const float* x_nchw,
                              const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                              void* layer4_out_nhwc, float* pooled, float momentum, float eps, float* moments,
                              const float* centres, void* stream) {
    CVCL_CHECK_DTYPE_TRUNK(dtype, "cvcl_resnext50_fwd");
    CVCL_CHECK_ARG(x_nchw && layers && workspace && layer4_out_nhwc && pooled, "cvcl_resnext50_fwd: null pointer");
    CVCL_CHECK_ARG(((uintptr_t)centres & 15) == 0, "cvcl_resnext50_fwd: centres must be 16-byte aligned");
    CVCL_CHECK_ARG(n_layers == kTrunkLayers, "cvcl_resnext50_fwd: expected 53 conv+bn layers, got %d", n_layers);
    CVCL_CHECK_ARG(B > 0 && H % 32 == 0 && W % 32 == 0, "cvcl_resnext50_fwd: H, W must be multiples of 32");
    const TrunkLayout ws(dtype, B, H, W, workspace);
    if (workspace_bytes < ws.bytes) {
        cvcl_set_error("cvcl_resnext50_fwd: workspace too small");
        return CVCL_EWORKSPACE;
    }
    // BatchNorm accumulators of the 53 layers (bf16 train mode: finalize-on-load), cleared once per pass ahead of the stem
    long long* acc = (training && dtype == CVCL_BF16) ? ws.acc : nullptr;
    if (acc && hipMemsetAsync(acc, 0, kTrunkLayers * kAccBytes, (hipStream_t)stream) != hipSuccess) {
        cvcl_set_error("cvcl_resnext50_fwd: cannot clear the BatchNorm accumulators");
        return CVCL_ELAUNCH;
    }
    int rc;
    if (!training) {
        const EvalAffineAll t = trunk_table<EvalAffineAll>(layers);
        for (int i = 0; i < kTrunkLayers; ++i)
            CVCL_CHECK_ARG(t.gamma[i] && t.beta[i] && t.rm[i] && t.rv[i], "cvcl_resnext50_fwd: layer %d lacks BatchNorm tensors", i);
        // eval mode in bf16 stores every raw conv output as y - running_mean unless the caller brings its own centres
        // ($CVCL_CENTRED_STORAGE=0: plain storage; fp32 keeps plain storage -- nothing to gain there)
        static const bool centred = cvcl_env_on("CVCL_CENTRED_STORAGE");
        float* own = (!centres && centred && dtype == CVCL_BF16) ? ws.centres : nullptr;
        if ((rc = cvcl_bn_eval_affine_all(t, eps, ws.affine, centres, own, stream))) return rc;
        if (own) centres = own;
    }
    const PassCtx ctx = {dtype, B, training, momentum, eps, ws.stats, ws.gram, stream};
    const BnLayers bn = {layers, ws.affine, moments, centres, acc};

    // ---- stem ----
    int h = H / 2, wd = W / 2;
    char* RAW = ws.buf[2];
    // (The fused stem, cvcl_stem_pool -- a statistics-only pass, then convolution + bn1 + relu + maxpool in one kernel; bit-identical,
    // -1.0 GB of traffic per step at B = 256 -- measured slower here: profiles/r05_ab_stem.txt, same box, C2 5.13 -> 5.22 ms.  The stem
    // convolution itself runs at 116 us for 30 GFLOP (LDS-gather-bound), so recomputing it costs more than the 411 MB it stops
    // writing; the API and its bit-identity test stay for when the convolution gets faster.)
    if ((rc = cvcl_stem_conv7x7(dtype, x_nchw, layers[0].w, RAW, ws.stats, kMaxStatsRows, centres, B, H, W, stream))) return rc;
    if ((rc = bn.finalize(ctx, 0, cvcl_stem_conv_stats_rows(dtype, B, H, W), (long)B * h * wd, 64))) return rc;
    if ((rc = cvcl_bn_relu_maxpool(dtype, RAW, bn.scale(0), bn.shift(0), ws.buf[0], B, h, wd, 64, stream))) return rc;
    h /= 2; wd /= 2;
    if ((rc = walk_blocks(B, h, wd, ws.buf, (char*)layer4_out_nhwc, [&](const BlockGeom& g, const BlockBufs<char>& io) {
             return bottleneck_fwd(ctx, g, io, bn.from(g.li));
         }))) return rc;
    return cvcl_avgpool(dtype, layer4_out_nhwc, pooled, B, h * wd, kMaxC, stream);
}

extern "C" int cvcl_resnext50_fwd(int dtype, int B, int H, int W, int training, const float* x_nchw,
                                  const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                                  void* layer4_out_nhwc, float* pooled, float momentum, float eps, const float* centres,
                                  void* stream) {
    return resnext50_fwd_impl(dtype, B, H, W, training, x_nchw, layers, n_layers, workspace, workspace_bytes, layer4_out_nhwc, pooled,
                              momentum, eps, nullptr, centres, stream);
}

// ------------------------------------------------------------------------------------------------
// Train-mode pass with the running-statistics update split off, for passes pipelined on two streams: a frozen trunk's
// consecutive passes are independent except for the BatchNorm running statistics (each pass normalises with its own batch
// statistics), so pass k+1 may run beside pass k -- each fills the other's tail rounds, dependent-launch gaps and
// MFMA-bound phases -- as long as the 53 EMA updates are applied in pass order.  The pass leaves (mean, unbiased variance) of
// every layer in `moments` ([53][2][2048] floats) and touches no BatchNorm buffer; cvcl_resnext50_apply_moments, enqueued by
// the caller behind the previous pass's apply (one event), performs the updates of cvcl_resnext50_fwd bit for bit.
extern "C" size_t cvcl_resnext50_moments_floats(void) { return (size_t)kTrunkLayers * kAffStride; }

extern "C" int cvcl_resnext50_fwd_deferred_stats(int dtype, int B, int H, int W, const float* x_nchw,
                                                 const cvcl_convbn_params* layers, int n_layers, void* workspace,
                                                 size_t workspace_bytes, void* layer4_out_nhwc, float* pooled, float eps,
                                                 float* moments, const float* centres, void* stream) {
    CVCL_CHECK_ARG(moments, "cvcl_resnext50_fwd_deferred_stats: moments is NULL");
    return resnext50_fwd_impl(dtype, B, H, W, 1, x_nchw, layers, n_layers, workspace, workspace_bytes, layer4_out_nhwc, pooled,
                              0.f, eps, moments, centres, stream);
}

extern "C" int cvcl_resnext50_apply_moments(const cvcl_convbn_params* layers, int n_layers, const float* moments, float momentum,
                                            void* stream) {
    CVCL_CHECK_ARG(layers && moments && n_layers == kTrunkLayers,
                   "cvcl_resnext50_apply_moments: expected 53 conv+bn layers and their moments");
    const ApplyMomentsAll t = trunk_table<ApplyMomentsAll>(layers);
    for (int i = 0; i < kTrunkLayers; ++i)
        CVCL_CHECK_ARG(t.rm[i] && t.rv[i], "cvcl_resnext50_apply_moments: layer %d lacks running statistics", i);
    return cvcl_bn_apply_moments_all(t, moments, momentum, stream);
}

// ------------------------------------------------------------------------------------------------
// Grouped train-mode pass (linear-probe scoring: the reference's eval_linear_decoding.py:53-57, 89-91 and
// eval_object_categories_linear_decoding.py:52-56, 90-92 never call .eval(), so each 4-image trial is normalised with that
// trial's own batch statistics).  The B = T * group images form T consecutive groups; every BatchNorm normalises each group
// on the group's own mean and biased variance, so each group's outputs are those of cvcl_resnext50_fwd(training = 1) run on
// its images alone.  The convolutions run through the same entries as the batch pass with their statistics output off;
// after each one bn_group_stats / bn_group_finalize form a per-group affine and the bn_group_* passes apply it.  fp32
// storage only (CVCL_F32, CVCL_F32X3); the running statistics are read and written by nothing.
// ------------------------------------------------------------------------------------------------
namespace {
bool grouped_dtype(int dtype) { return dtype == CVCL_F32 || dtype == CVCL_F32X3; }

// cvcl_resnext50_fwd_grouped: 5 activation buffers, bn_group_stats partials, the per-group affines of a block's 4 layers
struct GroupedLayout {
    float *buf[5], *part, *aff[4];                      // aff: per-group (scale [T][C], shift [T][C]) of kConv1 .. kDownsample
    size_t bytes;
    GroupedLayout(int B, int H, int W, int T, void* base = nullptr) {
        Regions r{(uintptr_t)base};
        for (float*& b : buf) b = r.take<float>(act_elems(B, H, W) * 4);
        part = r.take<float>(cvcl_bn_group_part_floats(T) * 4);
        for (float*& a : aff) a = r.take<float>((size_t)T * 2 * kMaxC * 4);
        bytes = r.end;
    }
};
}  // namespace

extern "C" size_t cvcl_resnext50_fwd_grouped_workspace_bytes(int dtype, int B, int H, int W, int group) {
    if (!grouped_dtype(dtype) || B <= 0 || group < 1 || B % group != 0 || H <= 0 || W <= 0) return 0;
    return GroupedLayout(B, H, W, B / group).bytes;
}

extern "C" int cvcl_resnext50_fwd_grouped(int dtype, int B, int H, int W, int group, const float* x_nchw,
                                          const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                                          void* layer4_out_nhwc, float* pooled, float eps, void* stream) {
    CVCL_CHECK_ARG(grouped_dtype(dtype), "cvcl_resnext50_fwd_grouped: dtype %d not supported (CVCL_F32 / CVCL_F32X3)", dtype);
    CVCL_CHECK_ARG(group >= 1, "cvcl_resnext50_fwd_grouped: group %d < 1", group);
    CVCL_CHECK_ARG(B > 0 && B % group == 0, "cvcl_resnext50_fwd_grouped: B = %d is not a multiple of group = %d", B, group);
    CVCL_CHECK_ARG(H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "cvcl_resnext50_fwd_grouped: H, W must be multiples of 32");
    CVCL_CHECK_ARG(x_nchw && layers && workspace && layer4_out_nhwc && pooled, "cvcl_resnext50_fwd_grouped: null pointer");
    CVCL_CHECK_ARG(n_layers == kTrunkLayers, "cvcl_resnext50_fwd_grouped: expected 53 conv+bn layers, got %d", n_layers);
    for (int l = 0; l < kTrunkLayers; ++l)
        CVCL_CHECK_ARG(layers[l].w && layers[l].gamma && layers[l].beta, "cvcl_resnext50_fwd_grouped: layer %d: null pointer", l);
    const int T = B / group;
    const GroupedLayout ws(B, H, W, T, workspace);
    if (workspace_bytes < ws.bytes) {
        cvcl_set_error("cvcl_resnext50_fwd_grouped: workspace too small");
        return CVCL_EWORKSPACE;
    }
    // layer l's raw output y ([T groups of rows_g rows, C]) -> its per-group affine in a (the bn_group_* launchers: csrc/bn.hip)
    auto group_bn = [&](int l, const float* y, long rows_g, int C, float* a) {
        return cvcl_bn_group_affine(y, T, rows_g, C, layers[l].gamma, layers[l].beta, eps, ws.part, a, stream);
    };
    int rc;
    // ---- stem: conv1 -> bn1 + relu + maxpool ----
    int h = H / 2, wd = W / 2;
    if ((rc = cvcl_stem_conv7x7(dtype, x_nchw, layers[0].w, ws.buf[2], nullptr, 0, nullptr, B, H, W, stream))) return rc;
    if ((rc = group_bn(0, ws.buf[2], (long)group * h * wd, 64, ws.aff[0]))) return rc;
    if ((rc = cvcl_bn_group_relu_maxpool(ws.buf[2], ws.aff[0], ws.buf[0], B, h, wd, 64, group, stream))) return rc;
    h = (h - 1) / 2 + 1; wd = (wd - 1) / 2 + 1;
    // ---- layer1 .. layer4 (torchvision Bottleneck.forward) ----
    auto block = [&](const BlockGeom& g, const BlockBufs<float>& io) -> int {
        const cvcl_convbn_params* L = layers + g.li;
        const long g_in = (long)group * g.h * g.w, g_out = (long)group * g.ho * g.wo;
        auto conv1x1 = [&](int j, const float* A, float* C) {
            const cvcl_gemm_args a = conv1x1_args(g, L, j, A, C);
            return cvcl_gemm(dtype, &a, stream);
        };
        int rc;
        if (g.first) {                                  // downsample 1x1 stride s: X -> RD [m_out, outc]
            if ((rc = conv1x1(kDownsample, io.X, io.RD))) return rc;
            if ((rc = group_bn(g.li + kDownsample, io.RD, g_out, g.outc, ws.aff[kDownsample]))) return rc;
        }
        // conv1 1x1: X -> R1 [m_in, width]; bn1 + relu in place
        if ((rc = conv1x1(kConv1, io.X, io.R1))) return rc;
        if ((rc = group_bn(g.li + kConv1, io.R1, g_in, g.width, ws.aff[kConv1]))) return rc;
        if ((rc = cvcl_bn_group_relu(io.R1, ws.aff[kConv1], T, g.m_in, g.width, g_in, stream))) return rc;
        // conv2 grouped 3x3 (stride here) on the normalised R1 (no affine on load): -> R2 [m_out, width]; bn2 + relu in place
        if ((rc = cvcl_gconv3x3(dtype, io.R1, nullptr, nullptr, L[kConv2].w, io.R2, nullptr, 0, nullptr, B, g.h, g.w, g.width, 32,
                                g.stride, stream))) return rc;
        if ((rc = group_bn(g.li + kConv2, io.R2, g_out, g.width, ws.aff[kConv2]))) return rc;
        if ((rc = cvcl_bn_group_relu(io.R2, ws.aff[kConv2], T, g.m_out, g.width, g_out, stream))) return rc;
        // conv3 1x1: R2 -> R3 [m_out, outc]
        if ((rc = conv1x1(kConv3, io.R2, io.R3))) return rc;
        if ((rc = group_bn(g.li + kConv3, io.R3, g_out, g.outc, ws.aff[kConv3]))) return rc;
        // bn3 + identity / bn(downsample) + relu -> dst
        return cvcl_bn_group_add_relu(io.R3, ws.aff[kConv3], g.first ? io.RD : io.X, g.first ? ws.aff[kDownsample] : nullptr, io.dst, T,
                                      g.m_out, g.outc, g_out, stream);
    };
    if ((rc = walk_blocks(B, h, wd, ws.buf, (float*)layer4_out_nhwc, block))) return rc;
    return cvcl_avgpool(dtype, layer4_out_nhwc, pooled, B, h * wd, kMaxC, stream);
}
