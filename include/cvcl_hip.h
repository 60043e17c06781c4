/* libcvcl_hip.so -- C ABI of the MI355X-native CVCL contrastive hot path.
 *
 * Drop-in boundary for the path SURVEY.md section 8 names.  The reference has no FFI: every
 * entry below replaces an *implicit ATen/cuDNN call* that the reference reaches through
 * torch.nn at the cited line (paths relative to the reference repo root), so a maintainer binds
 * it with ctypes from the same Python call site (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; every pointer is CALLER-OWNED DEVICE memory,
 *    contiguous in the documented layout; the library never allocates, never synchronises and
 *    only enqueues work on the passed hipStream_t (passed as void*; NULL = default stream).
 *  - return 0 on success, negative CVCL_E* otherwise; cvcl_last_error() gives the thread-local text.
 *  - scratch comes from the caller: cvcl_*_workspace_bytes() sizes it.
 *  - ONE DEVICE PER PROCESS (the launch model of the path: one rank per GPU).  Occupancy queries, CU counts and the raised
 *    dynamic-LDS attributes are cached per process on first use, for the device that is current then; a process that
 *    switches devices afterwards gets the first device's grid and statistics-row counts and unraised LDS limits there.
 *  - dtype: CVCL_F32 = fp32 storage + exact-fp32 MFMA (parity mode, the reference numerics);
 *           CVCL_BF16 = bf16 storage + bf16 MFMA with fp32 accumulation/statistics (perf mode);
 *           CVCL_F32X3 (ABI v7) = fp32 storage as CVCL_F32, with every trunk convolution's products formed from split-bf16 parts
 *           (x = x0 + x1 + x2, x_i bf16, six part products on the bf16 MFMA, fp32 accumulation: ~fp32 products at a fraction of
 *           the exact fp32 MFMA's time; csrc/gemm_split.hip for the 1x1 / downsample products, csrc/conv_split.hip for the stem
 *           and the grouped 3x3, BatchNorm partial rows fused).  Accepted by cvcl_pack_conv_weight / cvcl_packed_weight_bytes
 *           (the split parts: CVCL_PACK_DENSE [3][cout][cin] bf16, CVCL_PACK_STEM7 / _GCONV3 [3][cout / 32][steps][32][16] bf16),
 *           cvcl_gemm (A / C fp32, W a packed dense weight with ldw
 *           its row pitch inside a part; plain products + BN partial rows + row gather only, N % 128 == 0, K % 32 == 0;
 *           cvcl_gemm_stats_rows sizes the rows), cvcl_stem_conv7x7 / cvcl_stem_conv_stats_rows, cvcl_gconv3x3 /
 *           cvcl_gconv3x3_stats_rows, cvcl_resnext50_fwd / _fwd_deferred_stats / _workspace_bytes, cvcl_resnext50_block_fwd /
 *           _block_workspace_bytes, and the storage-side entries the trunk calls (cvcl_col_stats, cvcl_bn_relu_maxpool,
 *           cvcl_bn_add_relu, cvcl_bn_relu_apply, cvcl_avgpool: treated as CVCL_F32).  Every other entry that takes a dtype
 *           returns CVCL_EINVAL for it (and for any unknown value) before it enqueues anything; size queries return 0.
 *  - image activations inside the library are NHWC ("channels last"); the API takes the
 *    reference's NCHW fp32 images (multimodal_data_module.py:98-109) and hands back the layer4
 *    map in NHWC memory, which the host exposes as a logical NCHW tensor view.
 *
 * Run-time switches -- the ONLY environment variables the product library reads (once per process, csrc/api.cpp):
 *    variable               default  "0" means
 *    CVCL_CENTRED_STORAGE   on       plain (un-centred) bf16 storage of the raw convolution outputs (the round-2 numerics)
 *    CVCL_GEMM8W            on       cvcl_gemm never selects the 8-wave 256 x 256 kernel (everything on the 128 x 128 kernels)
 *    CVCL_GEMM_PRO          on       cvcl_gemm refuses the BN-prologue kernel (callers normalise the operand themselves)
 *    CVCL_FINALIZE_ON_LOAD  on       bf16 train-mode trunk: partial rows + a cvcl_bn_finalize launch behind EVERY convolution (the launch
 *                                    sequence of rounds 1-5) instead of accumulated statistics that the consumer of the raw tensor turns
 *                                    into its channels' affine itself ("BatchNorm accumulators" below; tests/test_finalize_on_load_gpu.py)
 *  The kernel-variant switches of the 8-wave GEMM live in tools/gemm_lab/.
 */
#ifndef CVCL_HIP_H
#define CVCL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVCL_ABI_VERSION 7

enum { CVCL_OK = 0, CVCL_EINVAL = -1, CVCL_ELAUNCH = -2, CVCL_EWORKSPACE = -3, CVCL_EUNSUPPORTED = -4 };
enum { CVCL_F32 = 0, CVCL_BF16 = 1, CVCL_F32X3 = 2 };
enum { CVCL_ACT_NONE = 0, CVCL_ACT_RELU = 1, CVCL_ACT_GELU = 2, CVCL_ACT_QUICK_GELU = 3 };
/* CVCL_ACT_QUICK_GELU: x sigmoid(1.702 x), the MLP activation of OpenAI's CLIP towers (the reference's --clip_eval baseline, eval.py:29-45,
 * 205-207, 224-226).  cvcl_gemm implements it in the bias / activation epilogues of the 8-wave kernel, of the direct-to-LDS bf16 kernel
 * and of the tiled kernel (fp32: v / (1 + expf(-1.702 v))); fp8, LayerNorm-folded, C_pre / G and CVCL_F32X3 blocks with it are refused
 * before anything is enqueued, and the small / 64 x 64 split fp32 kernels are not selected for it.                                  */
/* BatchNorm accumulators (round 6).  A convolution hands its per-channel batch statistics on either as partial ROWS (one per
 * workgroup, reduced by cvcl_bn_finalize) or, with stats_rows == CVCL_STATS_ACCUMULATE, by atomically ADDING them to a caller-zeroed
 * accumulator: int64 [8][2][N] (8 rows = one per XCD; [0] sums, [1] sums of squares), fixed point with 24 fractional bits -- integer
 * addition commutes, so the totals are bit-deterministic.  sum = (acc[0][0][n] + ... + acc[7][0][n]) / 2^24.  The bf16 train-mode
 * trunk (cvcl_resnext50_fwd*) uses them so that the consumer of a raw tensor forms its BatchNorm affine itself instead of waiting
 * for a cvcl_bn_finalize launch ($CVCL_FINALIZE_ON_LOAD). */
#define CVCL_STATS_ACCUMULATE (-1)

int cvcl_abi_version(void);
const char* cvcl_last_error(void);

/* Optional measurement aid (bench.py roofline): while enabled, every kernel launch is bracketed by
 * hipEvents recorded on the stream the kernel is launched on; cvcl_prof_collect synchronises them and
 * returns the summed device time and launch count per kernel class.  Off by default (zero overhead).  */
enum { CVCL_K_GEMM = 0, CVCL_K_GCONV = 1, CVCL_K_STEM = 2, CVCL_K_BN_FINALIZE = 3, CVCL_K_BN_ADD_RELU = 4,
       CVCL_K_MAXPOOL = 5, CVCL_K_AVGPOOL = 6, CVCL_K_HEAD = 7, CVCL_K_OTHER = 8, CVCL_K_ATTENTION = 9,
       CVCL_K_LAYERNORM = 10, CVCL_K_LSTM = 11, CVCL_K_GEMM_F32 = 12, CVCL_K_BN_APPLY = 13, CVCL_K_BN_BWD = 14,
       CVCL_K_WGRAD = 15, CVCL_K_GEMM8W = 16, CVCL_K_GEMM_PRO = 17, CVCL_K_NCLASSES = 18 };
int cvcl_prof_enable(int on);
int cvcl_prof_collect(double* ms_per_class, long* launches_per_class, int n_classes);
/* average event-to-event time (us) of the same bracket around a kernel that does nothing, over n launches: the share of
 * every bracket that is dispatch gap rather than kernel (a rocprofv3 kernel duration = bracket - this, to first order).  */
int cvcl_prof_null_bracket_us(void* stream, int n, double* avg_us);

/* ------------------------------------------------------------------------------------------
 * Text encoder, "embedding" branch.  Replaces nn.Embedding + sum/len
 * (multimodal/multimodal.py:496-503; table built at :311-312, padding_idx = 0).
 *   table [V,E] f32, tok [B,L] i64, len [B] i64
 *   -> ret [B,E] f32 = sum_l table[tok[b,l]] / len[b];  out_ble [B,L,E] f32 = table[tok] (may be NULL)
 * bwd: d_table [V,E] f32 (fully overwritten; row 0 = 0) from d_ret [B,E]; deterministic
 * (b,l)-ordered accumulation, no atomics.  Token ids outside [0,V) are an error the forward
 * reports by writing NaN into the affected rows (the reference raises an index error); the
 * backward gives such a position to no row (the ids are compared as int64: v + 2^32 is not v). */
int cvcl_embed_meanpool_fwd(const float* table, const int64_t* tok, const int64_t* len, float* ret,
                            float* out_ble, int B, int L, int E, int V, void* stream);
int cvcl_embed_meanpool_bwd(const float* d_ret, const int64_t* tok, const int64_t* len, float* d_table,
                            int B, int L, int E, int V, void* stream);

/* F.normalize(x, p=2, dim=-1, eps) rows (multimodal/multimodal.py:736,743).
 *   x [N,E] f32 -> y [N,E], norm [N] (the un-clamped L2 norm, kept for bwd)
 * bwd: dx = (dy - y (y.dy)) / max(norm,eps)   (dy / eps where norm < eps).                     */
int cvcl_l2norm_fwd(const float* x, float* y, float* norm, int N, int E, float eps, void* stream);
int cvcl_l2norm_bwd(const float* y, const float* norm, const float* dy, float* dx, int N, int E, float eps,
                    void* stream);

/* Similarity logits (multimodal/multimodal.py:755,783-787):
 *   logits_per_image [Ni,Nt] = (img [Ni,E] . txt [Nt,E]^T) * exp(*neg_log_temp)
 * logits_per_text is the transposed view of the same buffer (bitwise: match.t()*s).  fp32 MFMA.
 * bwd: d_img = s * dS . txt, d_txt = s * dS^T . img, d_neg_log_temp = sum(dS * logits) (NULL to skip).
 * workspace: cvcl_sim_logits_bwd_workspace_bytes.                                               */
int cvcl_sim_logits_fwd(const float* img, const float* txt, const float* neg_log_temp, float* logits,
                        int Ni, int Nt, int E, void* stream);
size_t cvcl_sim_logits_bwd_workspace_bytes(int Ni, int Nt, int E);
int cvcl_sim_logits_bwd(const float* img, const float* txt, const float* neg_log_temp, const float* logits,
                        const float* d_logits, float* d_img, float* d_txt, float* d_neg_log_temp,
                        int Ni, int Nt, int E, void* workspace, size_t workspace_bytes, void* stream);
/* The same restricted to a range of rows (data-parallel global negatives, SURVEY.md 8e: every rank evaluates the replicated
 * N_g x N_g loss on the all-gathered features and back-propagates through ITS OWN rows only):
 *   d_img_rows [ni, E] = s * dS[i0 : i0 + ni, :] . txt          (image rows i0 .. i0 + ni - 1)
 *   d_txt_rows [nt, E] = s * dS[:, t0 : t0 + nt]^T . img        (text rows  t0 .. t0 + nt - 1)
 *   d_neg_log_temp = sum(dS * logits) over the WHOLE matrix (identical on every rank).
 * Operands are read in place (K-major GEMM operands): no workspace.  cvcl_sim_logits_bwd = the full ranges.                  */
int cvcl_sim_logits_bwd_rows(const float* img, const float* txt, const float* neg_log_temp, const float* logits,
                             const float* d_logits, float* d_img_rows, float* d_txt_rows, float* d_neg_log_temp,
                             int Ni, int Nt, int E, int i0, int ni, int t0, int nt, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Symmetric InfoNCE with arange labels + accuracies + entropies in one pass over the logits
 * (multimodal/multimodal.py:801-818, multimodal/utils.py:106-108).
 *   logits [N,N] f32 (= logits_per_image; logits_per_text is its transpose)
 *   -> scalars[5] = {infonce, image_accuracy, text_accuracy, image_entropy, text_entropy}
 *      row_lse [N], col_lse [N] (log-sum-exp per row / column, kept for bwd)
 * bwd: d_logits [N,N] = *d_loss/(2N) * (softmax_rows + softmax_cols - 2 I).
 * workspace (fwd): cvcl_infonce_workspace_bytes(N).                                             */
size_t cvcl_infonce_workspace_bytes(int N);
int cvcl_infonce_fwd(const float* logits, int N, float* scalars5, float* row_lse, float* col_lse,
                     void* workspace, size_t workspace_bytes, void* stream);
int cvcl_infonce_bwd(const float* logits, const float* row_lse, const float* col_lse, const float* d_loss,
                     float* d_logits, int N, void* stream);

/* get_entropy(logits, dim=-1) (multimodal/utils.py:106-108): out[r] = -sum_j p log p of softmax(x[r,:]). */
int cvcl_row_entropy(const float* x, float* out, int R, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * MFMA GEMM with fused prologue/epilogue -- the 1x1 convolutions of torchvision's Bottleneck
 * (call site multimodal/multimodal.py:101), nn.Linear fc/head (:190-192), ViT qkv/proj/fc1/fc2
 * (multimodal/vision_transformer_dino_mugs.py:92-94,113-115) and the text transformer linears.
 *
 *   C[M,N] = act( A'[M,K] . W[N,K]^T * (exp(*exp_scale)) + bias[N] ) (+ R[M,N])
 *   A'     = A, or relu?(A * a_scale[K] + a_shift[K])  (BatchNorm+ReLU of the producer fused into
 *            the operand load), rows optionally gathered with a spatial stride (1x1 stride-2 conv)
 *   stats  = per-column sum / sum-of-squares of the stored C (BatchNorm batch statistics of this
 *            conv's output), one partial row per persistent block: stats[grid_m][2][N] f32
 * All matrices row-major with the given leading dimensions (elements).  dtype selects the storage
 * type of A, W, C, R.  A bf16 block rounds to bf16 where the unfused modules would store a tensor:
 * the operand A' after its prologue, the linear's output before the residual is added, and the
 * stored result, so with a residual C = round(round(act(...)) + R).                               */
typedef struct {
    const void* A; const void* W; void* C;
    int M, N, K, lda, ldw, ldc;
    /* optional operand prologue (NULL = none) */
    const float* a_scale; const float* a_shift; int a_relu;
    /* optional row gather: output row m = (b, oy, ox) reads input row (b, oy*stride, ox*stride) */
    int gather_ho, gather_wo, gather_hi, gather_wi, gather_stride;   /* gather_stride 0/1 = off */
    /* optional epilogue */
    const float* exp_scale; const float* bias; int act;
    const void* R; int ldr;
    float* stats; int stats_rows;    /* stats_rows = capacity (>= cvcl_gemm_stats_rows(dtype, args)); rows written = that value.
                                      * stats_rows == CVCL_STATS_ACCUMULATE (bf16): stats points to int64 accumulators [8][2][N] that the
                                      * launch ADDS its per-channel (sum, sum of squares) to -- see "BatchNorm accumulators" below */
    /* Bottleneck tail (bf16): C = relu(round(A'W^T) * c_scale[N] + c_shift[N] + (R | R * r_scale[N] + r_shift[N])).
     * With C == NULL and stats != NULL the product is not stored, only its column statistics (same rounding). */
    const float* c_scale; const float* c_shift; const float* r_scale; const float* r_shift;
    /* training epilogues of the ViT MLP (bf16): C_pre != NULL with act = GELU also stores the pre-activation u = round(acc + bias)
     * (C = round(gelu(u))); G != NULL multiplies the rounded product by gelu'(G) (G [M][ldg] = the saved u): the data gradient
     * through the GELU, C = round(round(A W^T) * gelu'(G)).  Both NULL for every other use. */
    void* C_pre; const void* G; int ldg;
    /* centred storage of a raw convolution output (bf16 and fp32): with centre != NULL the product is stored (and its
     * statistics taken, and the Bottleneck tail's c_scale / c_shift applied) as round(A'W^T - centre[n]).  Train-mode
     * BatchNorm is invariant under a per-channel shift of its input, so consumers that apply (scale, shift) on load need no
     * change; cvcl_bn_finalize adds the centre back into the running mean.  Only the convolution epilogues honour it (no
     * bias / activation / residual-only epilogue).  See "Centred storage" below.                                          */
    const float* centre;
    /* Bottleneck tail with the downsample branch RECOMPUTED (bf16, the BN-prologue kernel, K = 128): instead of reading the
     * stored branch through R, identity = round(A2[M,K2] . W2[N,K2]^T - centre2[n]) * r_scale[n] + r_shift[n] with A2 = the block
     * input and W2 = the 1x1 downsample weight, K2 = 64 (torchvision Bottleneck.downsample of layer1.0: nn.Conv2d(64, 256, 1) +
     * BatchNorm).  R must be NULL; the statistics behind r_scale / r_shift come from cvcl_conv1x1_gram(A2) + cvcl_bn_from_gram(W2)
     * (or a statistics-only cvcl_gemm(A2, W2, C = NULL)). */
    const void* A2; const void* W2; int K2, lda2, ldw2; const float* centre2;
    /* LayerNorm folded into the linear (bf16, the 8-wave kernel only; reference vision_transformer_dino_mugs.py:136-149:
     * x + attn(norm1(x)), x + mlp(norm2(x)) -- nn.LayerNorm feeding nn.Linear).
     *   consumer (ln_stats != NULL; bias / activation epilogue, no residual): A = the RAW rows x, W = W diag(gamma) (rounded to
     *     bf16 by the caller), ln_colsum[n] = sum_k W'[n][k] of that rounded matrix, bias[n] = b[n] + sum_k W[n][k] beta[k]
     *     (required), ln_stats[m] = (rstd_m, -mean_m rstd_m):  C = round(act(rstd acc - mean rstd ln_colsum[n] + bias[n])).
     *     ln_stats is fetched in 16-byte granules: it must be readable for an EVEN number of rows (M + (M & 1)).
     *   producer (row_part != NULL; bias + residual epilogue): additionally row_part[m][N / 64][2] f32 = (sum, sum of squares) of
     *     the STORED row over each 64-column strip; cvcl_row_stats_finalize reduces them to the next consumer's ln_stats.
     * cvcl_gemm_ln_supported tells whether cvcl_gemm routes these arguments to the kernel that honours them. */
    const float* ln_stats; const float* ln_colsum; float* row_part;
    /* K-major operands and fused row sums (fp32 only, round 5): the gradient GEMMs of the trainable tail -- nn.Linear backward
     * (dW = dY^T X, dX = dY W, db = sum_m dY; reference call sites multimodal/multimodal.py:192 fc, :553-573 text transformer) and of
     * the similarity logits (:755) -- read their operands as they lie in memory instead of through transposed copies:
     *   a_trans != 0: element (m, k) of A is at A[k * lda + m]   (A is stored [K][M]);  w_trans != 0: W[k * ldw + n] (stored [K][N]);
     *   a_rowsum [M] f32 (needs a_trans): a_rowsum[m] = sum_k A'[m][k] -- with A' = dY^T this is the bias gradient, produced by the
     *   weight-gradient GEMM's own operand loads (fixed summation order, deterministic).
     * No prologue / gather / statistics / BN-tail options with these. */
    int a_trans, w_trans; float* a_rowsum;
    /* f32_split != 0 (fp32 only, round 5): fp32 operands, arithmetic on the bf16 MFMA with every element split into two bf16 parts
     * (hi.hi + hi.lo + lo.hi, fp32 accumulation): products good to ~2^-16 relative, ~4x the exact-fp32 kernel's speed.  For the
     * trainable tail of the bf16 configurations (the text transformer's linears and their gradients; the reference under bf16
     * autocast runs them as plain bf16 GEMMs); the fp32 parity mode never sets it. */
    int f32_split;
} cvcl_gemm_args;
int cvcl_gemm_grid_m(int dtype, int M, int N, int has_prologue);   /* needs a GPU (occupancy query) */
int cvcl_gemm(int dtype, const cvcl_gemm_args* args, void* stream);
/* exact number of statistics rows cvcl_gemm writes for these arguments when given a buffer of at least that many rows
 * (args->stats / stats_rows are ignored); ONLY those rows are defined afterwards -- reduce exactly that many.  With a smaller
 * buffer sized by cvcl_gemm_grid_m the 128-tile kernel runs and writes cvcl_gemm_grid_m rows.  (The 8-wave and the
 * BN-prologue kernels write fewer rows than cvcl_gemm_grid_m: always size and reduce by this function.)  */
int cvcl_gemm_stats_rows(int dtype, const cvcl_gemm_args* args);
/* The 8-wave 256 (224) x 256 bf16 kernel the dispatcher of cvcl_gemm selects for the MFMA-bound shapes (ResNeXt layers 2-4 1x1
 * convolutions, ViT linears; N % 256 == 0, K % 128 == 0), callable directly with the same argument block.
 * epi 0 = convolution epilogue (round + BN partial sums; C may be NULL), epi 1 = bias / activation / residual.
 * cvcl_gemm8w_tile_rows: the tile height (256 or 224) the epi-0 launch uses for an [M, N] output; cvcl_gemm8w_stats_rows: the
 * number of BN-statistics rows it writes.                                                                                */
int cvcl_gemm8w(int epi, const cvcl_gemm_args* args, void* stream);
/* The bandwidth-bound form cvcl_gemm selects when the operand carries the producer's BatchNorm + ReLU (a_scale / a_shift /
 * a_relu) and K = 128 | 256, N % 256 == 0 (conv3 of ResNeXt layers 1-2 on the raw grouped-convolution output: torchvision
 * Bottleneck.forward conv3(relu(bn2(.)))): statistics only (C NULL), C + statistics, or the Bottleneck tail (c_scale ...).
 * Round 6: the first two epilogues also take the operand as stored (a_scale == a_shift == NULL); cvcl_gemm routes such a product
 * here from 2^17 rows up (conv1 of ResNeXt layer2.0: K = 256, N = 256, M = 802 816 at B = 256).                            */
int cvcl_gemm_pro(const cvcl_gemm_args* args, void* stream);
int cvcl_gemm_pro_supported(const cvcl_gemm_args* args);
int cvcl_gemm_pro_stats_rows(int M, int N);
int cvcl_gemm8w_supported(int M, int N, int K, int lda, int ldw, int ldc);
/* Co-scheduling hint (round 4): the 8-wave GEMM kernels (bf16 and e4m3) run one 160-KiB-LDS workgroup per CU, so a launch that
 * fills the chip keeps every other stream's kernels out until its last round.  A host that keeps TWO passes of a frozen trunk in
 * flight on two streams sets cus = half the chip: each launch then takes twice as long on half the CUs and the two passes really run
 * side by side (ViT-B/16, B = 256, two trunk streams: 12.1 -> 11.9 ms per step; the ResNeXt trunk is faster with full grids).
 * Process-global, read at launch time (one host thread per process, as everything here); 0 = all CUs; returns the previous value.
 * Results do not depend on it (tile order only), except that BN-statistics row counts do: cvcl_gemm8w_stats_rows follows it. */
int cvcl_set_gemm_cu_share(int cus);
/* 1 when cvcl_gemm(CVCL_BF16, args) runs the 8-wave kernel for these arguments (shape policy included), i.e. ln_stats / row_part
 * would be honoured; 0 otherwise (cvcl_gemm then refuses arguments that carry them: CVCL_EUNSUPPORTED).  No GPU needed. */
int cvcl_gemm_ln_supported(const cvcl_gemm_args* args);
/* LayerNorm row statistics for the folded form above.  cvcl_row_stats: x [rows][D] (row stride in elements) ->
 * out[row] = (rstd, -mean rstd), biased variance + eps as nn.LayerNorm; cvcl_row_stats_finalize: the producer's strip partials
 * row_part[rows][strips][2] (strips = D / 64) -> the same.  fp64 combination of fp32 sums. */
int cvcl_row_stats(int dtype, const void* x, long x_row_stride, float* out, long rows, int D, float eps, void* stream);
int cvcl_row_stats_finalize(const float* row_part, int strips, float* out, long rows, int D, float eps, void* stream);
int cvcl_gemm8w_tile_rows(int M, int N);
int cvcl_gemm8w_stats_rows(int M, int N);

/* Train-mode BatchNorm statistics of a 1x1 convolution's output WITHOUT forming the output (round 4, csrc/bn_gram.hip): torchvision
 * Bottleneck.forward bn3(conv3(relu(bn2(.)))) / downsample[1](downsample[0](x)), reached from multimodal/multimodal.py:101, where the
 * convolution runs fused with its consumer and its statistics are needed first.  With a' = relu?(A * a_scale + a_shift) rounded to bf16
 * (a_scale NULL: A as stored), cvcl_conv1x1_gram leaves G = sum_m a'[m] a'[m]^T (only its upper-triangle 32 x 32 tiles are computed) and
 * s = sum_m a'[m] in fp64 inside the workspace (*gram_out: G [K][K] row-major, then s [K]); cvcl_bn_from_gram turns them into what
 * cvcl_bn_finalize produces for y = a' W^T (W bf16 [N][ldw]): mean = w.s / M, var = w^T (G - s s^T / M) w / M, (scale, shift) of the
 * stored tensor y - centre, running statistics or deferred moments.  bf16 rows, K = 64 | 128 | 256; deterministic.               */
size_t cvcl_conv1x1_gram_workspace_bytes(int K);
int cvcl_conv1x1_gram(const void* A, int lda, long M, int K, const float* a_scale, const float* a_shift, int a_relu, void* workspace,
                      size_t workspace_bytes, const double** gram_out, void* stream);
int cvcl_bn_from_gram(const double* gram, int K, long count, const void* W, int ldw, int N, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                      float* scale, float* shift, float* moments, int moments_ld, const float* centre, void* stream);

/* out[c][r] = in[r][c], f32 (operand re-layout for the weight-gradient GEMMs). */
int cvcl_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
/* d_bias[n] = sum_m dY[m][n], f32. */
int cvcl_colsum_f32(const float* dY, float* d_bias, int M, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * ResNeXt-50 32x4d trunk = torchvision.models.resnext50_32x4d (third-party; reference call sites
 * multimodal/multimodal.py:96-102,155-158, multimodal/utils.py:207-209).  NHWC activations.
 * "raw" = convolution output before BatchNorm; every conv kernel emits per-channel sum / sumsq
 * partial rows stats[rows][2][C] of what it stored; cvcl_bn_finalize turns them into (scale, shift)
 * + running-stat EMA (nn.BatchNorm2d train mode: eps 1e-5, momentum 0.1, unbiased running var,
 * num_batches_tracked += 1); consumers apply scale/shift(+ReLU) on load.
 *
 * Centred storage.  A raw conv output whose per-channel batch mean is large next to its spread loses precision when it
 * is rounded to bf16 BEFORE BatchNorm subtracts the mean (the rounding error 2^-9 |y| becomes 2^-9 |y| / sigma of the
 * normalised value).  Every convolution entry therefore takes an optional per-output-channel `centre` c (fp32, device):
 * it stores round(y - c) and takes the statistics of THAT; BatchNorm(y - c) == BatchNorm(y), so (scale, shift) from
 * cvcl_bn_finalize apply to the stored tensor unchanged and the finalize adds c back where the true mean is needed
 * (running_mean, moments).  c only has to be within ~sigma of the batch mean: the host keeps the batch means of a
 * calibration pass (multimodal/resnext.py).  centre == NULL is c = 0 (plain storage).                               */
enum { CVCL_PACK_DENSE = 0, CVCL_PACK_STEM7 = 1, CVCL_PACK_GCONV3 = 2 };

typedef struct {
    const void* w;                 /* conv weight packed by cvcl_pack_conv_weight (dtype of the run) */
    const float* gamma; const float* beta;          /* BatchNorm weight / bias                       */
    float* running_mean; float* running_var; int64_t* num_batches_tracked;   /* updated when training */
} cvcl_convbn_params;

/* centre (nullable): the c the producer stored its output with; running_mean receives batch mean + c.
 * cvcl_bn_eval_affine: shift = beta - (running_mean - c) * scale, the eval-mode affine of a tensor stored as y - c.  */
int cvcl_bn_finalize(const float* stats, int rows, long count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                     float eps, float* scale, float* shift, const float* centre, int C, void* stream);
int cvcl_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, float* scale, float* shift, const float* centre, int C, void* stream);
int cvcl_col_stats_rows(long rows);
int cvcl_col_stats(int dtype, const void* x, long rows, int C, float* stats, int stats_rows, void* stream);

/* weights arrive in the reference layout (OIHW fp32, device) and are re-laid-out once per weight version */
size_t cvcl_packed_weight_bytes(int dtype, int kind, int cout, int cin_per_group, int k);
int cvcl_pack_conv_weight(int dtype, int kind, const float* w_oihw, void* out, int cout, int cin_per_group, int k,
                          void* stream);

/* conv1 7x7/2 pad 3, 3->64: x NCHW f32 [B,3,H,W] -> y NHWC raw [B,H/2,W/2,64] (+stats) */
int cvcl_stem_conv_stats_rows(int dtype, int B, int H, int W);
int cvcl_stem_conv7x7(int dtype, const float* x_nchw, const void* w_packed, void* y_nhwc, float* stats, int stats_rows,
                      const float* centre /* [64] or NULL */, int B, int H, int W, void* stream);
/* (bf16: y_nhwc == NULL = statistics only -- the first pass of the fused stem below.)
 * conv1 + bn1 + relu + maxpool in ONE pass (round 5; torchvision ResNet.forward conv1 -> bn1 -> relu -> maxpool, reached from
 * multimodal/multimodal.py:101): the raw [B,H/2,W/2,64] tensor is never written -- in train mode its BatchNorm statistics come from
 * a statistics-only cvcl_stem_conv7x7 pass, then this kernel recomputes the convolution and pools it out of LDS:
 * y NHWC bf16 [B, ceil(H/4), ceil(W/4), 64], bit-identical to cvcl_stem_conv7x7 + cvcl_bn_relu_maxpool.  bf16, W <= 252. */
int cvcl_stem_pool_supported(int dtype, int H, int W);
int cvcl_stem_pool(int dtype, const float* x_nchw, const void* w_packed, const float* scale, const float* shift,
                   const float* centre /* [64] or NULL */, void* y_nhwc, int B, int H, int W, void* stream);
/* relu(bn(x)) then maxpool 3x3/2 pad 1: [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C] */
int cvcl_bn_relu_maxpool(int dtype, const void* x, const float* scale, const float* shift, void* y, int B, int H, int W,
                         int C, void* stream);
/* grouped 3x3 conv pad 1 stride 1|2 on relu(x*a_scale+a_shift): [B,H,W,C] -> raw [B,Ho,Wo,C] (+stats).
 * a_scale == a_shift == NULL: plain convolution of x (no affine, no ReLU) -- the data-gradient form. */
int cvcl_gconv3x3_stats_rows(int dtype, int B, int H, int W, int C, int stride);
int cvcl_gconv3x3(int dtype, const void* x, const float* a_scale, const float* a_shift, const void* w_packed, void* y,
                  float* stats, int stats_rows, const float* centre /* [C] or NULL */, int B, int H, int W, int C, int groups,
                  int stride, void* stream);
/* out = relu(raw*scale+shift + (idn | idn*idn_scale+idn_shift)), [rows, C] */
int cvcl_bn_add_relu(int dtype, const void* raw, const float* scale, const float* shift, const void* idn,
                     const float* idn_scale, const float* idn_shift, void* out, long rows, int C, void* stream);
/* y = relu(x*scale+shift), [rows, C]; y may alias x */
int cvcl_bn_relu_apply(int dtype, const void* x, const float* scale, const float* shift, void* y, long rows, int C,
                       void* stream);
/* adaptive avgpool to 1x1 + flatten: [B,HW,C] -> [B,C] f32 */
int cvcl_avgpool(int dtype, const void* x, float* out, int B, int HW, int C, void* stream);

/* Whole trunk in one call: conv1..layer4 + avgpool.  layers[53] in torchvision state_dict order
 * (conv1; per block conv1, conv2, conv3, [downsample.0]).  training != 0: batch statistics + running
 * stat updates (what the reference does even with a frozen CNN: Lightning keeps .train()).
 * -> layer4_out_nhwc [B,H/32,W/32,2048] (dtype), pooled [B,2048] f32.
 * centres (nullable): [53][2048] fp32 = cvcl_resnext50_centres_floats(), layer l's storage centre at centres + 2048 l
 * ("Centred storage" above).  NULL = plain storage, except eval mode in bf16, where NULL selects c = running_mean (the
 * stored tensors are then y - running_mean; $CVCL_CENTRED_STORAGE=0 turns that default off).                         */
size_t cvcl_resnext50_workspace_bytes(int dtype, int B, int H, int W);
size_t cvcl_resnext50_centres_floats(void);
int cvcl_resnext50_fwd(int dtype, int B, int H, int W, int training, const float* x_nchw,
                       const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                       void* layer4_out_nhwc, float* pooled, float momentum, float eps, const float* centres, void* stream);
/* ONE Bottleneck of that trunk (torchvision.models.resnet.Bottleneck.forward, reached from multimodal.py:101), enqueued as
 * exactly the launch sequence cvcl_resnext50_fwd uses for it -- the unit the teacher-forced parity tests drive: feed the
 * oracle's block input, compare the block output.  stage 0..3 = layer1..layer4; first != 0 for the stage's first block
 * (downsample branch, stride 2 when stage > 0); layers = conv1, conv2, conv3[, downsample] of the block (3 or 4 entries);
 * x_nhwc [B,h,w,Cin] -> out_nhwc [B,h/s,w/s,256 << stage].                                                              */
size_t cvcl_resnext50_block_workspace_bytes(int dtype, int B, int h, int w, int stage);
int cvcl_resnext50_block_fwd(int dtype, int B, int h, int w, int stage, int first, int training, const void* x_nhwc,
                             const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                             void* out_nhwc, float momentum, float eps, const float* centres /* [n_layers][2048] or NULL */,
                             void* stream);
/* The train-mode pass with its BatchNorm running-statistics update split off (no counterpart in the reference, which runs
 * one pass at a time; same results).  Consecutive passes of a FROZEN trunk are independent except for those 53 EMA updates
 * (torch.nn.BatchNorm2d train mode, reached from multimodal.py:88-104 because Lightning keeps .train()), so a host may enqueue
 * pass k+1 on a second stream beside pass k and apply the updates in pass order:
 *   cvcl_resnext50_fwd_deferred_stats  = cvcl_resnext50_fwd(training = 1) that writes every layer's batch (mean, unbiased
 *       variance) to moments ([53][2][2048] floats = cvcl_resnext50_moments_floats()) and touches no BatchNorm buffer;
 *   cvcl_resnext50_apply_moments       = the 53 updates r <- (1 - momentum) r + momentum x and num_batches_tracked += 1 in one
 *       launch; enqueue it behind the previous pass's apply.  Bit-identical to the updates of cvcl_resnext50_fwd.          */
size_t cvcl_resnext50_moments_floats(void);
int cvcl_resnext50_fwd_deferred_stats(int dtype, int B, int H, int W, const float* x_nchw,
                                      const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                                      void* layer4_out_nhwc, float* pooled, float eps, float* moments, const float* centres,
                                      void* stream);
int cvcl_resnext50_apply_moments(const cvcl_convbn_params* layers, int n_layers, const float* moments, float momentum,
                                 void* stream);
/* Grouped train-mode pass (ABI v7, additive): the reference's linear-probe evaluation (eval_linear_decoding.py:53-57, 89-91;
 * eval_object_categories_linear_decoding.py:52-56, 90-92) never calls .eval(), so every 4-image trial runs the trunk with
 * that trial's own BatchNorm batch statistics.  B = T * group images in T consecutive groups: every one of the 53
 * BatchNorm layers normalises each group with the group's mean and biased variance over its group * h * w rows (eps, affine
 * as nn.BatchNorm2d in train mode), so each group's layer4_out_nhwc / pooled rows equal cvcl_resnext50_fwd(training = 1) on
 * those images alone.  The running statistics are neither read nor written (layers[l].running_* may be NULL).
 * CVCL_F32 and CVCL_F32X3 only (fp32 storage); CVCL_BF16, group < 1, B % group != 0, H or W not a multiple of 32, a null
 * pointer: CVCL_EINVAL before anything is enqueued.  The workspace query returns 0 for those.  Kernels: bn_group_stats
 * (centred two-pass partial moments), bn_group_finalize, bn_group_relu, bn_group_add_relu, bn_group_relu_maxpool.       */
size_t cvcl_resnext50_fwd_grouped_workspace_bytes(int dtype, int B, int H, int W, int group);
int cvcl_resnext50_fwd_grouped(int dtype, int B, int H, int W, int group, const float* x_nchw,
                               const cvcl_convbn_params* layers, int n_layers, void* workspace, size_t workspace_bytes,
                               void* layer4_out_nhwc, float* pooled, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * DINO ViT image encoder (multimodal/vision_transformer_dino_mugs.py:87-250), the one-layer text
 * transformer (multimodal/multimodal.py:553-573) and the LSTM text encoder (:513-552).  Linears run on
 * cvcl_gemm; these are the non-GEMM pieces.                                                        */
/* PatchEmbed unfold (vit:162,166): x NCHW f32 -> cols [B*np, Kpad] (k = c*p*p + ky*p + kx, zero padded) */
int cvcl_im2col_patches(int dtype, const float* x_nchw, void* cols, int B, int H, int W, int patch, int Kpad,
                        void* stream);
/* prepare_tokens (vit:232-243): h[b,0] = cls + pos[0]; h[b,1+i] = tok[b,i] + pos[1+i]; h [B,T,D]     */
int cvcl_vit_assemble_tokens(int dtype, const void* tok, const float* cls, const float* pos, void* h, int B, int T,
                             int D, void* stream);
/* nn.LayerNorm over the last dim; rows may be strided (x_row_stride elements); y is dtype or f32      */
int cvcl_layernorm(int dtype, const void* x, long x_row_stride, const float* gamma, const float* beta, float eps,
                   void* y, int y_is_f32, long rows, int D, void* stream);
/* softmax(q k^T * scale [+ key padding mask where key_tok == 0]) v;  qkv [B,T,3,heads,hd] -> out [B,T,heads*hd]
 * (vit:119-127; nn.MultiheadAttention inside nn.TransformerEncoderLayer).  bf16, hd = 64, no mask -> MFMA kernel. */
int cvcl_attention(int dtype, const void* qkv, const int64_t* key_tok, void* out, int B, int T, int heads, int head_dim,
                   float scale, void* stream);
/* the same attention under a causal mask: query t attends to keys 0..t, and only those products are computed (the text tower of
 * OpenAI's CLIP, which the reference scores as its --clip_eval baseline: eval.py:205-207, 224-226).  fp32 or bf16 storage, the generic
 * kernel in both (the text tower is a negligible share of a CLIP pass).  Same argument checks as cvcl_attention.                   */
int cvcl_attention_causal(int dtype, const void* qkv, void* out, int B, int T, int heads, int head_dim, float scale, void* stream);
/* CLIP's text pooling (eval.py:205-207, 224-226 through clip's encode_text): out[b,:] = LayerNorm(x[b, argmax_l tok[b,l], :]; gamma,
 * beta, eps) -- the end-of-text id is the largest of the vocabulary, the FIRST maximum wins (torch.argmax); one workgroup per sequence,
 * so ln_final costs B rows instead of B L.  x [B,L,W] f32, tok [B,L] int64, out [B,W] f32.                                          */
int cvcl_clip_text_pool(const float* x, const int64_t* tok, const float* gamma, const float* beta, float eps, float* out, int B, int L,
                        int W, void* stream);
/* same attention (bf16 qkv, head_dim 64, 32 < T), output written as e4m3 [B*T][heads*64] + e8m0 block scales tiled
 * [heads*64/128][B*T][4] -- cvcl_gemm_fp8_mx's MX input, so the fp8 projection needs no quantisation pass in between. */
int cvcl_attention_mx(const void* qkv, void* out8, void* out_block_scales, int B, int T, int heads, int head_dim, float scale,
                      void* stream);
/* Attention for a fine-tuned ViT (autograd of vision_transformer_dino_mugs.py:106-130): the forward above that also saves the
 * log-sum-exp of every row (lse [B][heads][T] fp32, log2 units), and the backward: d_qkv [B][T][3][heads][64] bf16 from
 * qkv, the forward output o and d_o ([B][T][heads*64] bf16).  Two kernels (queries own dQ; keys own dK, dV), probabilities
 * rebuilt from lse, no atomics: deterministic.  head_dim 64; 32 < T <= 288. */
int cvcl_attention_train(const void* qkv, void* out, float* lse, int B, int T, int heads, int head_dim, float scale, void* stream);
int cvcl_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, void* d_qkv, int B, int T, int heads,
                       int head_dim, float scale, void* stream);
/* LayerNorm backward on bf16 rows (32 lanes per row, D % 8 == 0, D <= 1024): dx = rstd (g - mean(g) - xhat mean(g xhat)) with
 * g = dy gamma, plus `add` (nullable: the residual-stream gradient that bypasses the norm); dy bf16 or fp32; per-group partial
 * sums of dgamma = sum dy xhat and dbeta = sum dy in partial [cvcl_layernorm_bwd_rows_partials(rows)][2][D] (reduce with
 * cvcl_colsum_f32: fixed order, deterministic).                                                                          */
int cvcl_layernorm_bwd_rows_partials(long rows);
int cvcl_layernorm_bwd_rows(const void* x, long x_row_stride, const float* gamma, const void* dy, int dy_is_f32, long dy_row_stride,
                            float eps, const void* add, void* dx, long dx_row_stride, float* partial, long rows, int D, void* stream);
/* GELU (erf form) on bf16: d_y == NULL -> y = gelu(u); else y = d_y * gelu'(u) (u = the saved pre-activation).  n % 8 == 0 */
int cvcl_gelu_bf16(const void* u, const void* d_y, void* y, long n, void* stream);
/* backward of cvcl_vit_assemble_tokens: d_tok [B][T-1][D] bf16 = the patch rows of dh [B][T][D]; d_pos [T][D] fp32 = sum over
 * the batch (its row 0 is also d_cls)                                                                                     */
int cvcl_vit_tokens_bwd(const void* dh, void* d_tok, float* d_pos, int B, int T, int D, void* stream);
/* fp32 fine-tuning of the ViT (csrc/vit_f32_train.hip; Lightning's default precision "32" under autograd of
 * vision_transformer_dino_mugs.py:87-149).  Every product on v_mfma_f32_32x32x2_f32 (exact fp32), no atomics, fixed-order
 * reductions: deterministic.  Each entry returns CVCL_EINVAL before it enqueues anything on a null pointer, a bad shape or a
 * limit it does not support.
 * Attention forward for training (vit:106-130 softmax(q k^T scale) v): qkv [B][T][3][heads][64] fp32 -> out [B][T][heads*64]
 * fp32 and lse [B][heads][T] fp32 in the log2 units of cvcl_attention_train.  head_dim 64, 32 < T <= 288, 16-byte aligned.   */
int cvcl_attention_train_f32(const float* qkv, float* out, float* lse, int B, int T, int heads, int head_dim, float scale, void* stream);
/* its backward (autograd of vit:106-130): d_qkv [B][T][3][heads][64] fp32, fully written; probabilities rebuilt from lse,
 * D_i = sum dO O in fp32; a dQ kernel that owns queries and a dK / dV kernel that owns keys.  Limits as the forward.           */
int cvcl_attention_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse, float* d_qkv, int B, int T, int heads,
                           int head_dim, float scale, void* stream);
/* LayerNorm backward on fp32 rows (autograd of nn.LayerNorm, vit:140/147): x, dy, add (nullable, dx's layout), dx fp32; partial
 * [cvcl_layernorm_bwd_rows_partials(rows)][2][D] as cvcl_layernorm_bwd_rows (reduce with cvcl_colsum_f32).  D % 4 == 0, D <= 1024. */
int cvcl_layernorm_bwd_rows_f32(const float* x, long x_row_stride, const float* gamma, const float* dy, long dy_row_stride, float eps,
                                const float* add, float* dx, long dx_row_stride, float* partial, long rows, int D, void* stream);
/* GELU (erf form, vit:99 nn.GELU) on fp32, the expression of cvcl_gemm's fp32 GELU epilogue: d_y == NULL -> y = gelu(u); else
 * y = d_y * gelu'(u).  n % 4 == 0, 16-byte aligned.                                                                         */
int cvcl_gelu_f32(const float* u, const float* d_y, float* y, long n, void* stream);
/* cvcl_vit_tokens_bwd on fp32 (autograd of prepare_tokens, vit:232-243): d_tok [B][T-1][D] fp32, d_pos [T][D] fp32 (batch sum,
 * row 0 = d_cls).  D % 4 == 0.                                                                                                */
int cvcl_vit_tokens_bwd_f32(const float* dh, float* d_tok, float* d_pos, int B, int T, int D, void* stream);
/* x[b,l,:] = table[tok[b,l]] (+ pos[l]) (multimodal.py:496, 561-563) */
int cvcl_embed_gather_pos(const float* table, const int64_t* tok, const float* pos, float* x, int B, int L, int E, int V,
                          void* stream);
/* ret[b,:] = sum over ALL L positions of x[b,l,:] / len[b] (multimodal.py:573) */
int cvcl_seq_sum_div(const float* x, const int64_t* len, float* ret, int B, int L, int E, void* stream);
/* one nn.LSTM step on precomputed gates [B,4H] (order i,f,g,o); rows with len <= t keep (h,c) and emit zeros */
int cvcl_lstm_cell(const float* gates, const int64_t* len, int t, float* h, float* c, float* out, int B, int L, int Hd,
                   void* stream);

/* Training side of the text encoders (the reference trains them under Lightning's .train(): dropout 0.1 in
 * nn.TransformerEncoderLayer, LockedDropout(dropout_i) ahead of the LSTM; multimodal/multimodal.py:46-53,513-573).
 * All f32, deterministic.  Dropout uses a counter-based hash of (seed, element index): the same call is the
 * backward.  shared_period > 0 shares the mask along a dimension of that extent (LockedDropout's [B,1,E] mask).  */
int cvcl_dropout(const float* x, const float* residual, float* y, long n, float p, unsigned long long seed,
                 long shared_period, long inner, void* stream);      /* y = dropout(x) (+ residual) */
/* LayerNorm backward: dx, plus dy*xhat per element (column-summed by cvcl_colsum_f32 into dgamma; dbeta = colsum(dy)) */
int cvcl_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, float* dx, float* dy_xhat, long rows,
                       int D, void* stream);
int cvcl_relu_bwd(const float* y, const float* dy, float* dx, long n, void* stream);
/* d_table[v] = sum of dx rows whose token is v, in position order; row 0 (padding_idx) = 0; fully overwritten */
int cvcl_embed_rows_bwd(const float* dx, const int64_t* tok, float* d_table, int n_pos, int E, int V, void* stream);
int cvcl_seq_sum_div_bwd(const float* d_ret, const int64_t* len, float* dx, int B, int L, int E, void* stream);
/* nn.MultiheadAttention core for short sequences (T <= 32) with key padding mask and probability dropout:
 * forward when out != NULL, backward when d_qkv != NULL (P is recomputed).  qkv [B,T,3,heads,hd] f32.            */
int cvcl_attention_small(const float* qkv, const int64_t* key_tok, const float* d_out, float* out, float* d_qkv, int B,
                         int T, int heads, int head_dim, float scale, float dropout_p, unsigned long long seed,
                         void* stream);
/* nn.LSTM step t that saves, in [B,L,.] layout (row b*L+t), the gate activations, c_t and h_{t-1} for BPTT; and the
 * BPTT step: d_gates rows b*L+t of [B,L,4H], dc updated in place, dh_carry = dh where the step was masked        */
int cvcl_lstm_cell_train(const float* gates, const int64_t* len, int t, float* h, float* c, float* out /*[B,L,H] or NULL*/,
                         float* gates_act, float* c_save, float* h_prev_save, int B, int L, int Hd, void* stream);
int cvcl_lstm_cell_bwd(const float* gates_act, const float* c_save, const int64_t* len, int t, const float* dh, float* dc,
                       float* d_gates, float* dh_carry, int B, int L, int Hd, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward side of the ResNeXt trunk for --finetune_cnn (multimodal/multimodal.py:175-179: the CNN's parameters keep
 * requires_grad, so autograd runs through torchvision's Bottlenecks).  Used by the autograd-composed fine-tuning
 * path; [rows, C] = NHWC activations flattened over pixels.                                              */
/* The elementwise entries below work on 16-byte channel chunks: 8 bf16 or 4 fp32 elements.  Wherever an entry takes a channel
 * count C or a flat element count n (cvcl_bn_apply, cvcl_bn_bwd, cvcl_add, cvcl_relu_mask, cvcl_maxpool3x3s2_idx,
 * cvcl_zero_stuff2), it must be a multiple of that chunk; anything else is refused with CVCL_EINVAL and nothing is launched.
 * (cvcl_avgpool_bwd, cvcl_transpose and cvcl_conv_wgrad_direct work per element and take any positive size.)                  */
/* y = x * scale + shift (ReLU if relu).  A thread keeps one channel chunk, so the chunks per row cc = C / chunk must be a power
 * of two, a divisor of 256 or a multiple of 256 (cc = 3 is refused, cc = 768 is served by a grid rounded to a multiple of 3). */
int cvcl_bn_apply(int dtype, const void* x, const float* scale, const float* shift, void* y, long rows, int C, int relu,
                  void* stream);
/* train-mode BatchNorm backward, g = dy * mask:
 *   mode 0: no mask | mode 1: [x*scale+shift > 0] (ReLU right after the BN; recomputed, y is not read) |
 *   mode 2: [out > 0], out = relu(bn(x) + identity) the Bottleneck output; g_out (optional) receives g = d identity.
 *   dbeta = sum g;  dgamma = sum g * xhat;  dx = gamma * rstd * (g - dbeta/n - xhat * dgamma/n)
 * partial: scratch [partial_rows >= cvcl_bn_bwd_partial_rows(dtype, rows, C)][2][C] f32, of which exactly that many rows are
 *   written;  coef: scratch [3][C] f32, left holding k1 = gamma*rstd, k2 = -k1*rstd*dgamma/n, k3 = -k1*dbeta/n - k2*mean
 *   (dx = k1*g + k2*x + k3).
 * C / chunk must be a power of two (C = 8, 16, 32, .. in bf16; 4, 8, 16, .. in fp32).  scale, shift, mean, rstd and coef are
 * read as 16-byte vectors and must be 16-byte aligned.  mode 1 needs scale and shift, mode 2 needs out; a mode outside 0..2, a
 * missing operand, a misaligned vector or partial_rows below the count above is refused with CVCL_EINVAL, nothing launched.  */
int cvcl_bn_bwd_partial_rows(int dtype, long rows, int C);
int cvcl_bn_bwd(int dtype, int mode, const void* x, const void* out, const void* dy, const float* scale, const float* shift,
                const float* mean, const float* rstd, const float* gamma, float* dgamma, float* dbeta, void* dx, void* g_out,
                long rows, int C, float* partial, int partial_rows, float* coef, void* stream);
/* batch mean and 1/sqrt(var_biased + eps) from the forward statistics rows (what bn_finalize normalised with; with centred
 * storage they are the moments of the STORED tensor y - c, which is what cvcl_bn_bwd needs next to that tensor).
 * centre_track (nullable, [C]): the c the producer used, updated in place to c + mean = the batch mean of y -- the storage
 * centre of the next step (a trunk that is being fine-tuned re-centres every step: its weights move).                 */
int cvcl_bn_batch_moments(const float* stats, int stats_rows, long count, float eps, float* mean, float* rstd,
                          float* centre_track, int C, void* stream);
/* OIHW f32 weight of the convolution that computes the data gradient of a grouped 3x3 conv (flip + in/out swap per group) */
int cvcl_gconv_weight_dgrad(const float* w, float* out, int C, int cin_per_group, void* stream);
int cvcl_transpose(int dtype, const void* in, void* out, long rows, int cols, void* stream);     /* out[c][r] = in[r][c] */
int cvcl_add(int dtype, const void* a, const void* b, void* y, long n, int relu, void* stream);  /* y = a + b (ReLU if relu) */
int cvcl_relu_mask(int dtype, const void* y, const void* dy, void* dx, long n, void* stream);    /* dx = dy where y > 0 */
/* max pool 3x3/2 pad 1, NHWC, with the arg-max recorded (idx [B,Ho,Wo,C] u8: window position ky*3 + kx in 0..8, the first
 * maximum in row-major window order, as torch): dy == NULL -> forward (reads x, writes out = pooled and idx); else backward
 * from idx (x unused, out = dx [B,H,W,C]: the sum of dy over the windows whose arg-max the pixel is)          */
int cvcl_maxpool3x3s2_idx(int dtype, const void* x, const void* dy, void* out, uint8_t* idx, int B, int H, int W, int C,
                          void* stream);
int cvcl_avgpool_bwd(int dtype, const float* d_pooled, void* dx, int B, int HW, int C, void* stream);
/* z[b,2oy,2ox,:] = dy[b,oy,ox,:], zeros elsewhere ([B,2Ho,2Wo,C]): data gradient of a stride-2 conv = stride-1 conv of z */
int cvcl_zero_stuff2(int dtype, const void* dy, void* z, int B, int Ho, int Wo, int C, void* stream);
/* dW[co][ci][ky][kx] (f32, reference OIHW layout) of a k x k (grouped) convolution, direct form */
int cvcl_conv_wgrad_direct(int dtype, const void* x, const void* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                           int cin_per_group, int k, int stride, int pad, int x_is_nchw_f32, void* stream);

/* Weight-gradient ("TN") GEMM: C[n][k] = sum_m A[m][n] * B[m][k], A [M, lda >= N], B [M, ldb >= K] row-major in the
 * run dtype, C [N, k_keep] f32 (k_keep <= K drops trailing padded columns).  1x1-conv weight gradient with A = dY,
 * B = X (NHWC, no transposed copies); the contraction is split over M with a fixed-order reduction (deterministic).
 * workspace >= cvcl_gemm_tn_workspace_bytes(dtype, M, N, K).                                             */
size_t cvcl_gemm_tn_workspace_bytes(int dtype, long M, int N, int K);
int cvcl_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, long M, int N, int K, float* C, int k_keep,
                 void* workspace, size_t workspace_bytes, void* stream);
/* nn.Linear backward in one pass over dY (bf16): C = A^T B as above and colsum[n] = sum_m A[m][n] (the bias gradient) */
size_t cvcl_gemm_tn_colsum_workspace_bytes(long M, int N, int K);
int cvcl_gemm_tn_colsum(const void* A, int lda, const void* B, int ldb, long M, int N, int K, float* C, int k_keep, float* colsum,
                        void* workspace, size_t workspace_bytes, void* stream);
/* nn.Linear backward in one pass over dY, fp32 (autograd of the ViT linears, vit:92-94 / 113-115): C [N][k_keep] = (A^T B)[:, :k_keep],
 * colsum [N] = column sums of A, on v_mfma_f32_32x32x2_f32; partial tiles over row chunks reduced in a fixed order (deterministic) */
size_t cvcl_gemm_tn_colsum_f32_workspace_bytes(long M, int N, int K);
int cvcl_gemm_tn_colsum_f32(const float* A, int lda, const float* B, int ldb, long M, int N, int K, float* C, int k_keep, float* colsum,
                            void* workspace, size_t workspace_bytes, void* stream);
/* grouped 3x3 (pad 1, stride 1|2) weight gradient, bf16 activations: dW [C][C/groups][3][3] f32 (reference OIHW); x and dy 16-byte aligned */
size_t cvcl_gconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C, int stride);
int cvcl_gconv3x3_wgrad(const void* x, const void* dy, float* dw, int B, int H, int W, int C, int groups, int stride,
                        void* workspace, size_t workspace_bytes, void* stream);
/* bf16 patch matrix of the 7x7/2 stem: col [B*H/2*W/2][160] (147 = 3*7*7 columns (c, ky, kx), zero-padded to 160);
 * stem weight gradient = cvcl_gemm_tn(A = dY [P,64], B = col, k_keep = 147)                              */
int cvcl_stem_im2col(const float* x_nchw, void* col_bf16, int B, int H, int W, void* stream);

/* embedding_type == "spatial", sim == "max" (multimodal/multimodal.py:770-787).  mm [Bi*HW, Bt*L] f32 is the match map
 * <image location, word> (one cvcl_gemm of the per-location image rows [Bi*HW, E] against the per-word text rows
 * [Bt*L, E]);  logits[i][t] = exp(*neg_log_temp) * sum_l max_p mm[(i,p)][(t,l)] / len[t]  (all L positions, as the
 * reference), arg [Bi, Bt*L] u8 = the winning location (first maximum).  HW <= 256.  The backward writes the dense
 * d_mm (zero except at the winners), from which d image rows = d_mm . text rows and d text rows = d_mm^T . image rows.
 * sim == "mean" needs no kernel of its own: mean over locations / words (cvcl_seq_sum_div) then cvcl_sim_logits.     */
int cvcl_bf16_to_f32(const void* x, float* y, long n, void* stream);      /* n % 8 == 0, 16-byte aligned */
/* its backward under --finetune_cnn (the gradient of the layer-4 map returns to the bf16 trunk, round to nearest even):
 * reference multimodal/multimodal.py:175-185 lets autograd run through nn.Sequential(trunk, Conv2d(2048, E, 1))          */
int cvcl_f32_to_bf16(const float* x, void* y, long n, void* stream);      /* n % 8 == 0, 16-byte aligned */
int cvcl_spatial_max_fwd(const float* mm, const int64_t* len, const float* neg_log_temp, float* logits, uint8_t* arg,
                         int Bi, int HW, int Bt, int L, void* stream);
int cvcl_spatial_max_bwd(const float* d_logits, const uint8_t* arg, const int64_t* len, const float* neg_log_temp,
                         const float* logits, float* d_mm, float* d_neg_log_temp /* nullable */, int Bi, int HW, int Bt, int L,
                         void* stream);

/* Language-model loss (lambda_lm > 0 configs; multimodal/multimodal.py:861-890, multimodal_lit.py:266-300).
 * token-wise F.cross_entropy(logits [R,V], labels [R], ignore_index, reduction "none"): loss[r] (0 for ignored rows), lse[r]
 * saved for the backward d_logits = (softmax - onehot) * d_loss.                                               */
/* BPTT with gradients on the per-step outputs: dh[b] += d_out[b][t] where len[b] > t (before cvcl_lstm_cell_bwd of step t) */
int cvcl_lstm_add_dout(float* dh, const float* d_out, const int64_t* len, int t, int B, int L, int Hd, void* stream);
/* remaining --text_encoder choices (multimodal.py:505-552).  cvcl_seq_reverse: y[b][t] = x[b][len-1-t] (t < len, else 0):
 * input / output permutation of the backward LSTM direction, self-adjoint.  cvcl_scale_add_f32: y = alpha * (a + b), b
 * nullable (mean of the two directions and its backward).  cvcl_cbow: window sum without the centre / (2 crange),
 * self-adjoint. */
int cvcl_seq_reverse(const float* x, const int64_t* len, float* y, int B, int L, int E, void* stream);
int cvcl_scale_add_f32(const float* a, const float* b, float alpha, float* y, long n, void* stream);
int cvcl_cbow(const float* x, float* y, int B, int L, int E, int crange, void* stream);

/* ---- f3: the training-time frame transform on the device ----------------------------------------------------------------
 * Replaces the per-frame PIL pipeline of multimodal_data_module.py:244-256 (RandomResizedCrop((224,224), scale (0.2,1)) ->
 * RandomApply([GaussianBlur([.1,2.])], p .5) (utils.py:94-103) -> RandomHorizontalFlip -> ToTensor -> Normalize (:57)) for a
 * whole batch in one launch, bit-identically to Pillow's integer pixel arithmetic (Resample.c bilinear with the down-scale
 * widened triangle filter, BoxBlur.c three-pass fractional box blur) and torch's fp32 (u8 / 255 - mean) / std.
 *   frames      uint8 [B][H][W][3]   decoded RGB frames (HWC), device memory
 *   crop        int32 [B][4]         top, left, h, w per frame (RandomResizedCrop.get_params order), device memory
 *   blur_sigma  fp32  [B]            <= 0 where RandomApply skipped the blur, device memory
 *   flip        int32 [B]            device memory
 *   mean, std3  3 HOST floats each
 *   out         fp32  [B][3][out_h][out_w]; out_u8 (nullable): uint8 [B][out_h][out_w][3], the image before ToTensor
 *   max_crop_h  upper bound of crop[:, 2] (H always works): sizes the LDS plan; boxes taller than ~500 rows at 224 x 224
 *               output do not fit the single-pass plan and are refused (CVCL_EARG)                                            */
int cvcl_augment_frames(const void* frames, int B, int H, int W, const int32_t* crop, const float* blur_sigma, const int32_t* flip,
                        const float* mean, const float* std3, void* out, int out_h, int out_w, void* out_u8, int max_crop_h,
                        void* stream);
/* The same transform through a frame index (ABI v7, additive): replaces the per-item frame lookup of the reference's dataset
 * (multimodal_saycam_data_module.py:107-122 -- pick frame_filenames[0] or a random one, Image.open(...).convert("RGB"), transform)
 * for a dataset whose frames were decoded once into one uint8 array that lives in HBM (multimodal/frame_store.py).
 *   store     uint8 [n_frames][H][W][3], device memory
 *   index     int64 [B], DEVICE memory: frame b is read at store + index[b] * H * W * 3, the offset formed in 64 bits (a full
 *             store is ~90 GB).  Values outside 0..n_frames-1 are clamped into the store on the device, so no index value can
 *             become a read outside it; reporting a bad index is the caller's job (FrameStore.transform raises IndexError)
 * Every other argument, the kernel and its arithmetic are cvcl_augment_frames'.  CVCL_EINVAL for what cvcl_augment_frames
 * refuses, a null store / index, or n_frames < 1; nothing is enqueued then.                                                  */
int cvcl_augment_frames_indexed(const void* store, int64_t n_frames, const int64_t* index, int B, int H, int W,
                                const int32_t* crop, const float* blur_sigma, const int32_t* flip, const float* mean,
                                const float* std3, void* out, int out_h, int out_w, void* out_u8, int max_crop_h, void* stream);

/* ---- evaluation-time frame transform (csrc/preprocess.hip) ------------------------------------------------------------------
 * The PIL transform every evaluation entry point of the reference runs per image, for a ragged batch in one launch:
 *   Resize((224, 224), BICUBIC) -> ToTensor -> Normalize      multimodal_lit.py:143-147 (the `preprocess` load_model returns; demo.py),
 *                                                             analysis_cvcl/alignment.py, embeddings.py:32-37,
 *                                                             generate_attention_maps.py:63-67,
 *                                                             object_categories_data_module.py:49-52, 106-109
 *   Resize(224, BICUBIC) -> CenterCrop(224) -> ToTensor -> Normalize     multimodal_data_module.py:259-266,
 *                                                             object_categories_data_module.py:38-45 (CLIP's transform)
 * bit-identically to Pillow's Resample.c (bicubic a = -0.5, support 2 widened by the down-scale; coefficients normalised in double
 * and rounded to 22 fractional bits; horizontal pass, then vertical pass, each rounded and clamped to uint8; a pass whose size does
 * not change is the identity) and torch's fp32 (u8 / 255 - mean) / std.  Only the out_h x out_w window of the resized image is
 * computed, which equals resize-then-crop bit for bit.
 *   frames       uint8, device: decoded RGB frames (HWC), each of its own size, packed into one buffer of frames_bytes bytes
 *   table        int64 [B][CVCL_PREPROCESS_TABLE_COLS], HOST: byte offset of the frame, source H, W, resized rh, rw, window
 *                origin ct, cl inside the resized image.  Validated before anything is enqueued
 *   table_dev    the same table in device memory (what the kernel reads)
 *   mean, std3   3 HOST floats each
 *   out          fp32 [B][3][out_h][out_w]; out_u8 (nullable): uint8 [B][out_h][out_w][3], the image before ToTensor
 * Sources up to 4096 x 4096, resized sizes up to 65536, windows up to 1024 x 1024, B up to 65535.  CVCL_EINVAL (with the reason in
 * cvcl_last_error) for a null pointer, B <= 0, a size out of range, a window that leaves the resized image, a frame that leaves the
 * buffer, or a filter whose tables do not fit LDS.                                                                              */
#define CVCL_PREPROCESS_TABLE_COLS 7
int cvcl_preprocess_frames(const void* frames, int64_t frames_bytes, const int64_t* table, const void* table_dev, int B,
                           const float* mean, const float* std3, void* out, int out_h, int out_w, void* out_u8, void* stream);
int cvcl_token_ce_fwd(const float* logits, const int64_t* labels, float* loss, float* lse, long R, int V, int ignore_index,
                      void* stream);
int cvcl_token_ce_bwd(const float* logits, const int64_t* labels, const float* lse, const float* d_loss, float* d_logits,
                      long R, int V, int ignore_index, void* stream);
/* the three masked means of multimodal_lit.py:284-300 and their token counts.  d_loss == NULL: forward (means[3],
 * counts[3] written); else backward: d_loss[r] = sum_k d_means[k] * mask_k[r] / counts[k].                      */
int cvcl_lm_loss_summaries(const float* loss, const int64_t* labels, const float* d_means, float* means, float* counts,
                           float* d_loss, int R, int pad, int sos, int eos, void* stream);

/* ------------------------------------------------------------------------------------------
 * FP8 (OCP e4m3) linears for the ViT encoder -- BASELINE configs[4] "fp8 MFMA weights/activations".
 * cvcl_quant_rows_fp8: q[r][:] = e4m3(y[r][:] / s[r]), s[r] = amax_k |y[r][k]| / 448 (1 for a zero row), where y = x or,
 *   with ln_gamma/ln_beta, nn.LayerNorm(x) (the vit blocks' norm1 / norm2 fused with the quantisation).  src_dtype: CVCL_BF16
 *   activations or CVCL_F32 (weights: one scale per output channel).  K % 8 == 0, K <= 4096.
 * cvcl_gemm_fp8: C[M,N] bf16 = act((A8 . W8^T) * a_scale[m] * w_scale[n] + bias[n]) (+ R), products on
 *   v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales, fp32 accumulation.  K % 128 == 0, N % 128 == 0.     */
int cvcl_quant_rows_fp8(int src_dtype, const void* x, long x_row_stride, const float* ln_gamma, const float* ln_beta,
                        float ln_eps, void* q, float* scale, long rows, int K, void* stream);
/* MX variants: a_block_scales = one e8m0 byte (2^(b-127)) per 32-element block of A instead of the per-row fp32 scale (the
 * scaled MFMA applies it in hardware), tiled [K/128][M][4] (block k/32 of row m at ((k/128)*M + m)*4 + (k/32)%4, so 32 rows'
 * words are contiguous); c8 / c_block_scales = e4m3 output [M][ldc8] + e8m0 scales in the same tiling [N/128][M][4]
 * (2^ceil(log2(amax/448)) per block) instead of bf16 C, ready to be the next GEMM's MX input -- no separate quantisation pass.
 * Large shapes (>= 96 tiles of 256 x 256 with a well-filled last round) run on the 8-wave kernel (csrc/gemm8f_kernel.h), which
 * fetches a tile's a_scale / a_block_scales in 16-byte granules: both must be readable up to the next multiple of 16 bytes
 * (a_scale: M rounded up to 4 floats; a_block_scales: 12 bytes past its end when M % 4 != 0).  Same results either way.            */
int cvcl_gemm_fp8_mx(const void* A8, const float* a_scale, const void* a_block_scales, int lda, const void* W8,
                     const float* w_scale, int ldw, void* C, int ldc, void* c8, void* c_block_scales, int ldc8,
                     const float* bias, int act, const void* R, int ldr, int M, int N, int K, void* stream);
/* The same with every option in one block (round 5), plus nn.LayerNorm FOLDED into the e4m3 linear it feeds (reference
 * vision_transformer_dino_mugs.py:136-149: x + attn(norm1(x)), x + mlp(norm2(x)); the bf16 form is cvcl_gemm_args.ln_stats):
 *   producer (row_part != NULL; proj / fc2: MX input, bias + residual): besides the bf16 rows C = round(acc sw + bias) + R the kernel
 *     writes their MX-quantised copy c8 / c_block_scales -- the RAW operand of the next qkv / fc1, e8m0 per 32 elements, no row-wide
 *     amax needed -- and row_part[m][N / 64][2] = (sum, sum of squares) of the stored row per 64-column strip (cvcl_row_stats_finalize
 *     turns them into ln_stats);
 *   consumer (ln_stats != NULL; qkv / fc1: MX input = those raw rows): W8 = e4m3(W diag(gamma)) with row scales w_scale,
 *     ln_colsum[n] = w_scale[n] * sum_k W8[n][k], bias[n] = b[n] + sum_k W[n][k] beta[k], ln_stats[m] = (rstd, -mean rstd):
 *     y = act(rstd (A8 . W8^T) w_scale - mean rstd ln_colsum + bias), to bf16 C or (c8 != NULL) to MX output.  8-wave kernel only:
 *     cvcl_gemm_fp8_ln_supported(M, N, K).  ln_stats readable for an even number of rows.
 * The 24 LayerNorm + row-quantise passes of a ViT-B (1.0 ms of an 8.2 ms step at B = 256) go; cvcl_quant_rows_mx quantises the
 * assembled tokens once per forward.                                                                                          */
typedef struct {
    const void* A8; const float* a_scale; const void* a_block_scales; int lda;
    const void* W8; const float* w_scale; int ldw;
    void* C; int ldc; void* c8; void* c_block_scales; int ldc8;
    const float* bias; int act; const void* R; int ldr;
    int M, N, K;
    const float* ln_stats; const float* ln_colsum; float* row_part;
} cvcl_gemm_fp8_args;
int cvcl_gemm_fp8_ex(const cvcl_gemm_fp8_args* args, void* stream);
int cvcl_gemm_fp8_ln_supported(int M, int N, int K);
/* bf16 rows [rows][K] (K % 128 == 0) -> e4m3 q [rows][K] + e8m0 block scales tiled [K / 128][rows][4] (one per 32 elements; the
 * quantiser of the MX-output epilogues, bit for bit). */
int cvcl_quant_rows_mx(const void* x, long x_row_stride, void* q, void* block_scales, long rows, int K, void* stream);
int cvcl_gemm_fp8(const void* A8, const float* a_scale, int lda, const void* W8, const float* w_scale, int ldw, void* C, int ldc,
                  const float* bias, int act, const void* R, int ldr, int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grad-CAM attention maps of the flat ResNeXt encoder (csrc/gradcam.hip).  Replace the forward + backward per image of
 * gradCAM (multimodal/attention_maps.py:125-165) and gradCAM_with_act_and_grad (:112-122).  With f = fc(avgpool(A)) the gradient
 * at the layer-4 map A is the same at every position, so every (image, target) map is one contraction over the map's channels:
 *   cam[n, m, p] = relu((R - s[n, m] U[n, p]) / (max(norm[n], eps) hw)),  R = sum_c P[m, c] A[n, p, c],  U = sum_c Q[n, c] A[n, p, c]
 * (normalised features: P = T W, Q = n^ W, s = n^ . t, norm = ||f||; below eps the s U term drops, as in cvcl_l2norm_bwd), or
 * relu(R / hw) with Q = s = norm = NULL.  map [N, HW, C] (NHWC, the trunk's layer-4 output) f32 or bf16, P [M, C] f32,
 * Q [N, C] f32, s [N, M] f32 (row-major over ALL M targets), norm [N] f32; C % 32 == 0, map / P / Q 16-byte aligned.
 * Exact-fp32 MFMA in both storage modes (R and s U cancel where a target is close to the feature).  Modes:
 *   CVCL_GRADCAM_ALL          k = 0:      cam [N, M, HW]  (every image with every target)
 *   CVCL_GRADCAM_BLOCK_IMAGE  M = N k:    cam [N, k, HW]  (image n with targets n k .. n k + k - 1; k = 1 is the diagonal)
 *   CVCL_GRADCAM_BLOCK_TEXT   N = M k:    cam [M, k, HW]  (target j with images j k .. j k + k - 1)
 * Profiling class CVCL_K_HEAD.  The hook bridge's avgpool backward (d_map = d_pooled / hw) is cvcl_avgpool_bwd.             */
enum { CVCL_GRADCAM_ALL = 0, CVCL_GRADCAM_BLOCK_IMAGE = 1, CVCL_GRADCAM_BLOCK_TEXT = 2 };
int cvcl_gradcam_pairs(int dtype, const void* map, int N, int HW, int C, const float* P, int M, int mode, int k, const float* Q,
                       const float* s, const float* norm, float eps, float* cam, void* stream);
/* F.interpolate(x, (H, W), mode='bicubic', align_corners=False) (attention_maps.py:158-163): x [maps, h, w] f32 -> y [maps, H, W]
 * f32 (16-byte aligned), torch's source coordinates, clamped taps and A = -0.75, any sizes with w <= 4096.  CVCL_K_OTHER.    */
int cvcl_bicubic_resize(const float* x, float* y, int maps, int h, int w, int H, int W, void* stream);
/* gradCAM_with_act_and_grad (attention_maps.py:112-122) for any layer: act, grad [N, C, HW] logical, each f32 or bf16 and each
 * NCHW-contiguous (nhwc = 0) or channels-last (nhwc = 1) in memory -> cam [N, HW] f32 = relu(sum_c mean_p(grad[n, c]) act[n, c, p]).
 * C <= 8192.  CVCL_K_OTHER.                                                                                                  */
int cvcl_gradcam_act_grad(int act_dtype, const void* act, int act_nhwc, int grad_dtype, const void* grad, int grad_nhwc, float* cam,
                          int N, int C, int HW, void* stream);

/* ------------------------------------------------------------------------------------------
 * Self-attention maps of the DINO ViT (csrc/vit_maps.hip; vision_transformer_dino_mugs.py:252-259 get_last_selfattention).
 * softmax(q k^T * scale) of vit:123-124, written out: qkv [B][T][3][heads][hd] (dtype f32 or bf16)
 * -> probs [B][heads][q_rows][T] fp32 for queries 0 .. q_rows-1 (q_rows = T: the whole matrix; 1: the CLS row).
 * hd = 64: MFMA route (fp32: v_mfma_f32_32x32x2_f32, exact; bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulation), one workgroup per
 * (image, head, 128 queries), key tiles of 64 streamed through LDS (any T), two passes (running max / sum, then the stores), no
 * T x T scratch, no atomics, fixed reduction order: deterministic.  qkv 16-byte aligned; probs needs no alignment beyond 4 bytes.
 * Other hd (hd % 4 == 0, hd <= 128): a plain fp32 VALU route.  CVCL_EINVAL before anything is enqueued on a null pointer, q_rows
 * outside 1 .. T, a dtype other than CVCL_F32 / CVCL_BF16, non-positive sizes or another hd.  CVCL_K_ATTENTION.               */
int cvcl_attention_probs(int dtype, const void* qkv, float* probs, int B, int T, int heads, int head_dim, float scale, int q_rows,
                         void* stream);
/* The CLS query's attention over the patch tokens: probs [B][heads][1][T] (cvcl_attention_probs with q_rows = 1) ->
 * out [B][T-1] = the mean over the heads (mean != 0; summed h = 0 first, then / heads) or out [B][heads][T-1] = a copy without
 * the CLS column (mean == 0).  T > 1; out must not alias probs.  CVCL_K_OTHER.                                                 */
int cvcl_cls_attention_maps(const float* probs, float* out, int B, int heads, int T, int mean, void* stream);
/* Attention rollout (Abnar & Zuidema 2020; the reference's ViT has none, so the formula below is the specification).
 * cvcl_attention_head_fuse (csrc/vit_maps.hip): qkv of ONE block as cvcl_attention_probs takes it -> fused [B][T][T] fp32,
 *   F[b] = fuse_h softmax(q k^T * scale)[b, h],  fuse = CVCL_FUSE_MEAN (the sum in head order, times 1 / heads once), MAX or MIN.
 * The softmax passes are those of cvcl_attention_probs (same routes, same limits: hd = 64 MFMA, other hd % 4 == 0 <= 128 VALU, qkv
 * 16-byte aligned on the MFMA route); one workgroup owns a [128 queries][T] tile of F[b] (VALU: one wave per row), visits the heads
 * in index order and folds each into its own elements of the tile, which stays in the L2: no [B][heads][T][T] intermediate, no
 * atomics, two calls give the same bits.  CVCL_EINVAL as cvcl_attention_probs, and on an unknown fuse.  CVCL_K_ATTENTION.
 * cvcl_attention_rollout (csrc/vit_rollout.hip): fused [n_layers][B][T][T] fp32 (layer 0 = the earliest block) ->
 *   out [B][q_rows][T] fp32 = the first q_rows rows of  A^_{n_layers-1} . A^_{n_layers-2} ... A^_{start_layer},
 *   A^_l = (F_l + I) / rowsum(F_l + I)  (the row sum is computed: it is 2 only for MEAN).
 * A^ is formed on the fly; one workgroup per (image, 8 rows; 1 row at q_rows = 1), the row vectors in LDS, r'[j] = sum_i r[i] A^[i][j]
 * summed over i = 0 .. T-1 in order with fp64 accumulators, the reads of F coalesced along j.  Deterministic; row q does not
 * depend on q_rows.  1 <= n_layers, 0 <= start_layer < n_layers, 1 <= q_rows <= T <= 960 (LDS: 17 T floats); out must not alias
 * fused.  No workspace.  CVCL_K_ATTENTION.                                                                                     */
enum { CVCL_FUSE_MEAN = 0, CVCL_FUSE_MAX = 1, CVCL_FUSE_MIN = 2 };
int cvcl_attention_head_fuse(int dtype, const void* qkv, float* fused, int B, int T, int heads, int head_dim, float scale, int fuse,
                             void* stream);
int cvcl_attention_rollout(const float* fused, float* out, int n_layers, int B, int T, int start_layer, int q_rows, void* stream);
/* The discard_ratio variant of the rollout (Gildenblat's vit-explain; csrc/vit_discard.hip): between the fuse and the chain, the k
 * weakest attentions of every fused matrix are zeroed in place.  fused [n_mats][T][T] fp32, n_mats = n_layers B; per matrix,
 * flattened row-major to M = T T elements: S = the first k indices of a stable ascending sort of the values (ties go to the lowest
 * flat index); every element with its index in S \ {0} becomes +0.0, every other element keeps its bits.  Flat index 0 (CLS -> CLS)
 * is never zeroed but counts towards k.  The caller computes k = int(T T discard_ratio).  Exact: a radix select over the uint32 bit
 * patterns (non-negative floats order as unsigned integers), one workgroup per matrix, integer LDS histograms, no global atomics,
 * no workspace; two calls give the same bits.  Negative or NaN values: unspecified result, same accesses.  CVCL_EINVAL before
 * anything is enqueued on a null pointer, n_mats <= 0, T outside 1 .. 4096, k outside 0 .. T T - 1; k == 0 returns CVCL_OK without
 * a launch.  CVCL_K_ATTENTION.                                                                                                  */
int cvcl_attention_discard(float* fused, int n_mats, int T, long k, void* stream);

/* ------------------------------------------------------------------------------------------
 * Beam-search decoding of the LSTM language model (csrc/textgen.hip; its LSTM cells: csrc/lstm.hip).  Replaces the reference's LanguageModel.beam_search_decode
 * (multimodal/multimodal.py:893-960) over beam_search (multimodal/beam_search.py:232-703): per decode step the torch composition
 * of grow_topk / grow_alive / grow_finished (:418-611) plus the host `.item()` of the stop test (:613-667) becomes one launch.
 *
 * cvcl_beam_step: step i (0 <= i < T, T = decode_length) for B items of K beams over a vocabulary of V, one workgroup per item.
 *   logits [B K, V] f32 (output layer, bias included); alive / finished log-probs and scores are ping-pong pairs [B, K] f32 (step i
 *   reads *_in, writes *_out); alive_seq, fin_seq [B, K, T + 1] int64 and fin_flags [B, K] int32 are updated in place (columns
 *   0..i + 1); h, c [B K, Hd] f32: the rows of each new beam's parent are gathered from *_in into *_out; next_tok [B K] int64.
 *   The step first evaluates the stop test (stop_early) for the whole batch from *_in: every item's max finished score above its
 *   alive_lp[:, 0] / ((5 + T) / 6)^alpha.  When it holds, the step only copies *_in to *_out and atomically lowers *steps to i, so
 *   a stopped decode stays stopped and *steps (initialised to T by the caller) is the reference's final loop index.
 *   Otherwise: scores = (log_softmax(logits) + alive_lp) / lp, lp = ((5 + i + 1) / 6)^alpha rounded to fp32; the top 2K of the K V
 *   scores ordered by (score desc, flat index asc) -- ties go to the lower index; then grow_alive (top K of score + flag * -1e7)
 *   and grow_finished (top K of [finished K ; score + (1 - flag) * -1e7]), both with the same tie rule.  eos_id marks a finished
 *   candidate.  Limits: 1 <= K <= CVCL_BEAM_MAX_K, 2K <= V, 1 <= T <= CVCL_BEAM_MAX_T, no null pointers, distinct ping-pong
 *   buffers; anything else is CVCL_EINVAL with nothing written.  CVCL_K_HEAD.
 * cvcl_beam_finalize: per item, finished sequences and scores if any finished flag is set, else the alive ones (:683-703), into
 *   out_seq [B, K, T + 1] int64 and out_scores [B, K] f32.  The caller trims to *steps + 1 columns.  CVCL_K_HEAD.
 * cvcl_lstm_cell_tok: the decode step's LSTM cell on N beam rows: gates [N, 4 Hd] = h W_hh^T, G [V, 4 Hd] = table W_ih^T + b_ih + b_hh
 *   computed once per decode; row tok[n] of G is added and the cell (gate order i, f, g, o as nn.LSTM) updates h, c [N, Hd] in
 *   place (the reference's inputs_to_outputs, multimodal.py:391-417).  A token outside [0, V) leaves its row unchanged.
 *   CVCL_K_LSTM.                                                                                                                 */
enum { CVCL_BEAM_MAX_K = 16, CVCL_BEAM_MAX_T = 128 };
int cvcl_beam_step(const float* logits, int B, int K, int V, int T, int step, double alpha, int eos_id, const float* alive_lp_in,
                   float* alive_lp_out, const float* fin_scores_in, float* fin_scores_out, int64_t* alive_seq, int64_t* fin_seq,
                   int32_t* fin_flags, const float* h_in, const float* c_in, float* h_out, float* c_out, int Hd, int64_t* next_tok,
                   int32_t* steps, void* stream);
int cvcl_beam_finalize(int B, int K, int T, const int64_t* alive_seq, const float* alive_lp, const int64_t* fin_seq,
                       const float* fin_scores, const int32_t* fin_flags, int64_t* out_seq, float* out_scores, void* stream);
int cvcl_lstm_cell_tok(const float* gates, const float* G, const int64_t* tok, int V, float* h, float* c, int N, int Hd,
                       void* stream);
/* BPTT step t = 0 of the training LSTM started from (h0, c0) (captioning: the connector's state, reference init_hidden
 * :671-688 feeding train_greedy): cvcl_lstm_cell_bwd at t = 0 with c_{-1} = c0 [B, Hd] f32 instead of zeros; dc leaves as the
 * gradient wrt c0, and dh_{-1} = d_gates[t = 0] W_hh + dh_carry (the caller's GEMM) is the gradient wrt h0.  CVCL_K_LSTM.          */
int cvcl_lstm_cell_bwd_first(const float* gates_act, const float* c_save, const float* c0, const int64_t* len, const float* dh,
                             float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-word Grad-CAM of the captioning LM (csrc/lstm.hip, csrc/head.hip).  Replaces the loop of the reference's
 * analysis_tools/multimodal_visualization.py:26-41 -- one loss[0, step - 1].backward(retain_graph=True) per word and image -- by
 * one multi-seed BPTT sweep: every (caption b, position p) is a seed row whose chain d loss[b, p] / d (h0, c0) runs over the saved
 * gate activations of caption b.  The seed state dh, dc is seed-major ([L][B][Hd]: block p = the chains that start at position p),
 * so the chains alive at step s (p >= s) are the contiguous tail from block s, and a step is this entry on that tail + one cvcl_gemm
 * (dh <- d_gates W_hh + dh_carry, M = rows).  Nothing keeps a d_gates history: no weight gradient is wanted.
 *
 * cvcl_lstm_cell_bwd_seeds: the cell backward of step s on rows = B n_active seed rows (dh, dc, d_gates [rows, 4 Hd], dh_carry
 *   [rows, Hd] all start at the tail's first row); row r reads gates_act / c_save (the [B, L, .] buffers cvcl_lstm_cell_train saved)
 *   at row b L + s, b = r % B, and len[b].  Per element the arithmetic of cvcl_lstm_cell_bwd (bit for bit), with c_{-1} = c0 [B, Hd]
 *   at s = 0 when c0 != NULL (cvcl_lstm_cell_bwd_first) and zeros otherwise; rows with len[b] <= s give d_gates = 0, dh_carry = dh
 *   and keep dc.  d_out [B, L, Hd] (nullable): the first B rows JOIN at this step -- their dh is d_out[b L + s] where len[b] > s and 0
 *   elsewhere, their dc is 0, and neither dh nor dc is read for them (no separate copy / clear launch).  dc is updated in place.
 *   fp32, four hidden units per lane (16-byte loads and stores): Hd % 4 == 0 and every buffer 16-byte aligned.  Refused with
 *   CVCL_EINVAL before anything is enqueued: null pointers, Hd, s outside [0, L), rows not a multiple of B or more than (L - s) B,
 *   c0 at s > 0.  CVCL_K_LSTM.
 * cvcl_l2norm_bwd_seeds: cvcl_l2norm_bwd for gradient rows that share an image's (y, norm): dy [K B, E] seed-major (row p B + b)
 *   -> dx [B K, E] image-major (row b K + p, the target order of CVCL_GRADCAM_BLOCK_IMAGE), y [B, E], norm [B]; y = norm = NULL:
 *   the reordering alone.  One launch for all K seeds (K launches of cvcl_l2norm_bwd otherwise).  dx must not alias dy.  CVCL_K_HEAD. */
int cvcl_lstm_cell_bwd_seeds(const float* gates_act, const float* c_save, const float* c0, const int64_t* len, int s,
                             const float* d_out, float* dh, float* dc, float* d_gates, float* dh_carry, int B, int L, int Hd, long rows,
                             void* stream);
int cvcl_l2norm_bwd_seeds(const float* y, const float* norm, const float* dy, float* dx, int B, int K, int E, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Nearest-neighbour searches between two frame sets (csrc/neighbors.hip).  Replace the torch compositions of the reference's
 * leakage check analysis_cvcl/duplicates.py; neither writes a queries x base matrix.  Both validate everything before they enqueue
 * anything (null pointers, Nq / Nb / D / C / HW out of range, strides below D, a workspace that is too small or not 16-byte aligned,
 * one group array without the other: CVCL_EINVAL, cvcl_last_error names the argument), enqueue on the caller's stream only, use no
 * atomics (partials per workgroup in the caller's workspace, merged in a fixed order: reproducible), and send ties to the LOWER index.
 * NaN inputs are not supported.  Chunked base sets: call once per chunk with idx_offset = the chunk's first row and accumulate = 1
 * from the second chunk on; the outputs then hold the running best (chunks in ascending order give the one-shot result bit for bit).
 *
 * cvcl_nn_cosine: F.cosine_similarity(a[:, None, :], b[None, :, :], dim=-1) + max / argmax over the base rows (duplicates.py:805-809
 *   over all training frames, :576-577 + :604-605 per category).  q [Nq, D] f32 (row stride ldq >= D), base [Nb, D] f32 (row stride
 *   ldb >= D); cos(i, j) = q_i . b_j / (max(|q_i|, eps) max(|b_j|, eps)) (torch: eps = 1e-8) -> best_cos [Nq] f32 = max_j,
 *   best_idx [Nq] int64 = idx_offset + argmax_j.  q_group / base_group (int32 per row, both or neither): only pairs of equal group
 *   are eligible -- the per-category search in one launch; a query without an eligible base row gets index -1 and -inf (or keeps
 *   what it had, with accumulate).  Products are exact fp32 (v_mfma_f32_32x32x2_f32), summed in chains of 128 k that are then added
 *   in fp32; norms and the final division in double, one rounding to fp32.  Zero rows give cosine 0.  CVCL_K_HEAD.
 * cvcl_nn_l1_u8: torch.sum(torch.abs(eval_img - train_images), dim=(1, 2, 3)) + min / argmin (duplicates.py:993-1002) on 8-bit frames.
 *   q [Nq, C, HW] uint8 planar, base [Nb, C, HW] uint8 (both 4-byte aligned; 16-byte aligned with HW % 16 == 0 for the wide loads),
 *   w [C] double HOST values (read during the call).  Per pair and channel S_c = sum_p |q[c, p] - b[c, p]| as an exact integer
 *   (v_sad_u8), d = S_0 w_0 + S_1 w_1 + ... in double, left to right, products and sums rounded separately -> best_dist [Nq] double
 *   = min_j, best_idx [Nq] int64 = idx_offset + argmin_j (-1 and +inf without an eligible base frame), best_sums [Nq, C] uint32 = the
 *   winner's S_c (may be NULL).  With w_c = 1 / (255 std_c) d is the reference's distance between ToTensor + Normalize frames (the
 *   mean cancels), without the rounding of its 150 528 fp32 terms.  Limits: 1 <= C <= 4, HW % 4 == 0, HW 255 < 2^32.  CVCL_K_OTHER. */
size_t cvcl_nn_cosine_workspace_bytes(int Nq, int Nb, int D);
int cvcl_nn_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps, const int32_t* q_group,
                   const int32_t* base_group, int64_t idx_offset, int accumulate, float* best_cos, int64_t* best_idx, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t cvcl_nn_l1_u8_workspace_bytes(int Nq, int Nb, int C);
int cvcl_nn_l1_u8(const uint8_t* q, const uint8_t* base, int Nq, int Nb, int C, int HW, const double* w, const int32_t* q_group,
                  const int32_t* base_group, int64_t idx_offset, int accumulate, double* best_dist, int64_t* best_idx,
                  uint32_t* best_sums, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * k nearest neighbours and the weighted k-NN vote (csrc/neighbors.hip).  The reference has only the k = 1 case (duplicates.py:805-809,
 * cvcl_nn_cosine above); the k closest training frames per evaluation frame and the vote over them are the weighted k-NN protocol of
 * the DINO evaluation (defaults k = 20, T = 0.07).  Both entries validate everything before they enqueue anything (CVCL_EINVAL,
 * cvcl_last_error names the argument), enqueue on the caller's stream only and use no atomics: two calls give the same bits.
 *
 * cvcl_knn_cosine: per query the k eligible base rows of largest cosine, sorted by (cosine descending, index ascending) -> top_cos
 *   [Nq, k] f32, top_idx [Nq, k] int64 = idx_offset + row; slots beyond the eligible count hold -inf / -1.  q, base, ldq, ldb, eps,
 *   q_group / base_group, idx_offset as cvcl_nn_cosine.  accumulate = 1: the outputs already hold a valid sorted list (of earlier
 *   chunks, all of lower index) and are merged with this chunk; chunks in ascending order give the one-shot lists bit for bit.  The
 *   cosine of a pair is cvcl_nn_cosine's expression on the same tile walk (norms in double, exact fp32 products, chains of 128 k,
 *   float(double(dot) inv_q inv_b)): it depends neither on k nor on the split nor on the chunking, and k = 1 gives cvcl_nn_cosine's
 *   result bit for bit.  No queries x base matrix is written: the base tiles are split over workgroups as in cvcl_nn_cosine, and each
 *   (split, query) keeps ONE sorted list of k (value, row) pairs IN THE CALLER'S WORKSPACE (at k = 256 the 128 lists of a workgroup
 *   are 256 KiB: they do not fit beside the staging tiles in LDS); only its k-th entry, the threshold, sits in LDS.  A tile's
 *   cosines go through LDS once; a wave reads the 64 candidates of one query, and only where one of them beats the threshold under
 *   the tie rule (or the list is not full) it merges them into the list by rank, one read and one write of the list.  A second
 *   kernel merges the splits' lists, and the previous outputs under accumulate, split by split.  Limits: 1 <= k <= CVCL_KNN_MAX_K.
 *   Workspace: cvcl_knn_cosine_workspace_bytes (0 = refused sizes) -- the norms and splits x Nq x k pairs.  CVCL_K_HEAD.
 * cvcl_knn_vote: scores[i][c] = sum over the entries j of list i whose base row has label c of exp(top_cos[i][j] / temperature)
 *   (temperature == 0: weight 1, the plain majority vote); weights and sums in double, added in list order, one rounding to fp32.
 *   pred[i] = the arg-max of the double sums, the lowest class on a tie; -1 when no entry counts.  An entry is skipped, never
 *   dereferenced, if its index is negative or >= Nb, or its label lies outside [0, C).  top_cos / top_idx [Nq, k] as cvcl_knn_cosine
 *   leaves them, base_label [Nb] int32 -> scores [Nq, C] f32, pred [Nq] int64.  Limits: 1 <= k <= CVCL_KNN_MAX_K,
 *   1 <= C <= CVCL_KNN_MAX_CLASSES, Nb >= 1, temperature finite and >= 0.  CVCL_K_HEAD. */
#define CVCL_KNN_MAX_K 256
#define CVCL_KNN_MAX_CLASSES 4096
size_t cvcl_knn_cosine_workspace_bytes(int Nq, int Nb, int D, int k);
int cvcl_knn_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, int k, float eps,
                    const int32_t* q_group, const int32_t* base_group, int64_t idx_offset, int accumulate, float* top_cos,
                    int64_t* top_idx, void* workspace, size_t workspace_bytes, void* stream);
int cvcl_knn_vote(const float* top_cos, const int64_t* top_idx, int Nq, int k, const int32_t* base_label, int64_t Nb, int C,
                  float temperature, float* scores, int64_t* pred, void* stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval ranks (csrc/neighbors.hip, ABI v7 additive): how far down the list of all base rows, sorted by cosine, a query's own row
 * stands -- Recall@K, median rank.  The reference has no retrieval evaluation; this is the third consumer of the cosine tile walk.
 *
 * cvcl_rank_cosine: query i's positives are the base rows j with base_key[j] == q_key[i], every other row is a negative (both key
 *   arrays are required; a single target per query is base_key[j] = j, q_key[i] = target[i]).  thr_cos [Nq] f32 / thr_idx [Nq] int64 =
 *   the query's best positive and its global row: what cvcl_nn_cosine returns with q_group = q_key, base_group = base_key over the
 *   WHOLE base set (the caller runs that search first; -1 / -inf without a positive).  rank [Nq] int64 = the number of negatives j of
 *   this call with cos(i, j) > thr_cos[i], or cos(i, j) == thr_cos[i] and idx_offset + j < thr_idx[i]: the 0-based position of the best
 *   positive in a stable descending sort with the other positives removed.  thr_idx[i] < 0: rank[i] = -1, also under accumulate.
 *   accumulate = 1 adds this chunk's count to what rank holds; the counts are integers, so chunks in ANY order give the one-shot ranks.
 *   cos(i, j) is cvcl_nn_cosine's expression on the same tile walk (norms in double, exact fp32 products, chains of 128 k,
 *   float(double(dot) inv_q inv_b)): a pair's cosine has the bits the threshold has, which is what makes the comparison meaningful.
 *   q, base, ldq, ldb, eps, idx_offset and the ranges of Nq / Nb / D as cvcl_nn_cosine.  No list and no matrix: each lane counts for
 *   its queries in a register; the counts are reduced over lanes and waves, written per (split, query) into the workspace and summed
 *   by a second kernel (no atomics).  Everything is validated before anything is enqueued (null pointers, sizes, strides below D, a
 *   workspace that is too small or not 16-byte aligned, accumulate outside {0, 1}: CVCL_EINVAL, cvcl_last_error names the argument);
 *   work is enqueued on the caller's stream only; NaN inputs are not supported.  Workspace: cvcl_rank_cosine_workspace_bytes
 *   (0 = refused sizes).  CVCL_K_HEAD. */
size_t cvcl_rank_cosine_workspace_bytes(int Nq, int Nb, int D);
int cvcl_rank_cosine(const float* q, int ldq, const float* base, int ldb, int Nq, int Nb, int D, float eps, const int32_t* q_key,
                     const int32_t* base_key, const float* thr_cos, const int64_t* thr_idx, int64_t idx_offset, int accumulate,
                     int64_t* rank, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual-hash duplicates (csrc/phash.hip, ABI v7 additive): the first half of the reference's analysis_cvcl/duplicates.py, "exact
 * and approximate duplicates" -- the 16 x 16 average hash of a frame, and per evaluation hash the closest training hash, by Hamming
 * distance and by the reference's own measure, fuzz.ratio of the two hashes written as decimal strings.  All three entries validate
 * everything before they enqueue anything (null pointers, counts, sizes and strides out of range, one group array without the other, a
 * workspace that is too small or not 16-byte aligned: CVCL_EINVAL, cvcl_last_error starts with the entry's name and names the
 * argument), enqueue on the caller's stream only, use no atomics (the base rows are split over workgroups, whose partial results go
 * through the caller's workspace to a merge kernel that walks them in a fixed order: two calls give the same bits) and send ties to
 * the LOWER index.  Everything is integer arithmetic: the results are exact.  CVCL_K_OTHER.
 *
 * cvcl_ahash_u8: ahash (duplicates.py:28-41) in the project's integer definition.  frames: N 8-bit RGB frames of H x W, addressed as
 *   frames[n stride_n + c stride_c + y stride_y + x stride_x] (element strides: planar [N, 3, H, W] is (3 H W, H W, W, 1),
 *   interleaved [N, H, W, 3] is (H W 3, 1, 3 W, 3), a crop of a larger tensor keeps its parent's strides).  Grey g = (19595 R +
 *   38470 G + 7471 B + 32768) >> 16 (ITU-R 601, Pillow's convert("L")).  Resize to 16 x 16, bilinear at half-pixel centres without
 *   antialiasing (cv2.resize's default): per axis of n source pixels and cell d, num = (2 d + 1) n - 16, i0 = num >> 5, w1 = num - 32 i0,
 *   w0 = 32 - w1, i1 = min(i0 + 1, n - 1); v = sum over the 2 x 2 taps of wy wx g (an exact integer, scaled by 1024), the cell value
 *   r = (v + 512) >> 10.  Bit i = 16 y + x is set when 256 r_i >= sum_j r_j (the reference's `resized >= resized.mean()`).
 *   -> hash [N, 4] int64 bit patterns, word w holding bits 64 w .. 64 w + 63 (bit 255 is the sign bit of word 3); cells [N, 256]
 *   int32 = the r (may be NULL).  One 256-thread workgroup per frame, one thread per cell, 12 byte loads per thread (3 072 bytes
 *   of a frame are read, whatever its size), the sum through LDS, one ballot per wave is one output word.  Limits: N >= 1, H, W >= 16,
 *   strides >= 1.  The reference decodes to grey inside libjpeg and rounds inside OpenCV: a grey level or a rare cell may differ by
 *   one from cv2's; this definition has not been compared with cv2.
 * cvcl_hamming_nn: q [Nq, 4], base [Nb, 4] int64 bit patterns -> best_dist [Nq] int32 = min_j popcount(q_i xor b_j), best_idx [Nq]
 *   int64 = the lowest j attaining it.  q_group / base_group (int32 per row, both or neither): only pairs of equal group are
 *   eligible; a query without an eligible base row gets index -1 and distance 257.  A lane owns one query in registers and walks
 *   the base hashes of its workgroup's range, which every lane reads at the same address.  Workspace:
 *   cvcl_hamming_nn_workspace_bytes (0 = refused sizes) -- splits x Nq (distance, row) pairs.
 * cvcl_digit_ratio_nn: the scan of duplicates.py:333-342.  q [Nq, ld], base [Nb, ld] uint8 strings over the alphabet 0..9 (digit
 *   values, not characters), q_len [Nq], base_len [Nb] int32 lengths, groups as above -> best_ratio [Nq] int32 = max_j ratio(q_i, b_j),
 *   best_idx [Nq] int64 = the lowest j attaining it, where ratio = round_half_even(200 LCS / (la + lb)) is thefuzz's fuzz.ratio
 *   (the normalised indel similarity), formed in integers by quotient and remainder.  A maximum of 0, or no eligible row, gives
 *   index -1 and ratio 0 (the reference scans from max_distance = 0 with a strict >).  LCS is the bit-parallel recurrence
 *   V = (V + (V & M)) | (V & ~M) over two 64-bit words with carry, M the query's match mask of the base string's digit (built once
 *   per query, in LDS); LCS = the zero bits among the low la bits of V.  Limits: 1 <= ld <= CVCL_DIGITS_MAX; lengths are device
 *   data and are clamped to [0, ld] where they are read (a length of 0 matches nothing); bytes above 9 are not supported (they
 *   match nothing).  A 256-bit hash has at most 78 digits.  Workspace: cvcl_digit_ratio_nn_workspace_bytes (0 = refused sizes).
 *   This definition has not been compared with thefuzz. */
#define CVCL_AHASH_SIDE 16
#define CVCL_AHASH_WORDS 4
#define CVCL_DIGITS_MAX 128
int cvcl_ahash_u8(const uint8_t* frames, int N, int H, int W, long stride_n, long stride_c, long stride_y, long stride_x, int64_t* hash,
                  int32_t* cells, void* stream);
size_t cvcl_hamming_nn_workspace_bytes(int Nq, int Nb);
int cvcl_hamming_nn(const int64_t* q, const int64_t* base, int Nq, int Nb, const int32_t* q_group, const int32_t* base_group,
                    int32_t* best_dist, int64_t* best_idx, void* workspace, size_t workspace_bytes, void* stream);
size_t cvcl_digit_ratio_nn_workspace_bytes(int Nq, int Nb);
int cvcl_digit_ratio_nn(const uint8_t* q, const int32_t* q_len, const uint8_t* base, const int32_t* base_len, int Nq, int Nb, int ld,
                        const int32_t* q_group, const int32_t* base_group, int32_t* best_ratio, int64_t* best_idx, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image-text alignment analysis (csrc/alignment.hip): the arithmetic of the reference's analysis_cvcl/alignment.py,
 * analysis_cvcl/embeddings.py:106-118 and analysis_tools/representation_similarity.py.  fp32 in and out (the Pearson moments: double),
 * contiguous rows.  Every entry validates everything before it enqueues anything (null pointers, sizes out of range, a workspace that
 * is too small or not 16-byte aligned: CVCL_EINVAL, cvcl_last_error names the argument) and enqueues on the caller's stream only.  No
 * floating-point atomics: the order of every sum is fixed by the shapes (and, for the class means, the labels), so two calls on the
 * same inputs give the same bits whatever the addresses.
 *
 * cvcl_class_mean_f32: np.mean(all_image_features[idxs], axis=0) per category (alignment.py:106-110; embeddings.py:88-90).
 *   x [N, D] f32, label [N] int32 in [0, C) (any order, classes of any size) -> mean [C, D] f32 and count [C] int32.  Sums in double
 *   (one rounding to fp32 after the division).  A class without rows gets count 0 and a zero row; rows whose label lies outside
 *   [0, C) are left out.  Limits: N < 2^24, D <= 2048, C <= 4096.  Workspace: cvcl_class_mean_workspace_bytes (0 = refused sizes)
 *   -- the row indices sorted by class and the histograms that sort them.  CVCL_K_OTHER.
 * cvcl_cosine_matrix_f32: out[i, j] = a_i . b_j / (max(|a_i|, eps) max(|b_j|, eps)), a [M, D], b [K, D] -> out [M, K]: the value of
 *   F.cosine_similarity(F.normalize(a_i), F.normalize(b_j), dim=0) (alignment.py:148-161, :182-195) and of cosine_matrix
 *   (representation_similarity.py:5-12).  Products are exact fp32 (v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32), the four
 *   partial sums of an element, the norms and the division are in double, one rounding to fp32.  a == b (the same pointer; then
 *   M == K) is allowed and gives an exactly symmetric matrix: one triangle is computed and written twice.  Zero rows give 0.
 *   Limits: M, K <= 4096, D <= 2048.  The grid follows M and K (16 x 16 outputs per workgroup below 256 tiles of 32 x 32).  CVCL_K_HEAD.
 * cvcl_triu_pearson_f32: scipy.stats.pearsonr(A[np.triu_indices(C, k=1)], B[np.triu_indices(C, k=1)]) (alignment.py:230-232;
 *   rsa_of_dissim_matrices, representation_similarity.py:30-39).  A, B [C, C] f32 -> out [6] doubles ON THE DEVICE: n = C (C - 1) / 2,
 *   r, mean_a, mean_b, var_a, var_b (population variances).  Centred in double: per workgroup the means of its rows, then the
 *   second moments about them; the partials are merged in a fixed tree.  A side whose values are all equal gives r = NaN (a value,
 *   as scipy returns it).  Limits: 3 <= C <= 4096.  Workspace: cvcl_triu_pearson_workspace_bytes.  CVCL_K_OTHER.
 * cvcl_paired_l2_f32: d_i = || x_i - y_i + eps ||_2 = F.pairwise_distance(x_i, y_i, p=2) (embeddings.py:106-111; torch: eps = 1e-6).
 *   x, y [C, D] f32 -> d [C] f32; differences and sums in double.  Limits: C <= 4096, D <= 2048.  CVCL_K_OTHER. */
size_t cvcl_class_mean_workspace_bytes(int N, int D, int C);
int cvcl_class_mean_f32(const float* x, const int32_t* label, int N, int D, int C, float* mean, int32_t* count, void* workspace,
                        size_t workspace_bytes, void* stream);
int cvcl_cosine_matrix_f32(const float* a, const float* b, int M, int K, int D, float eps, float* out, void* stream);
size_t cvcl_triu_pearson_workspace_bytes(int C);
int cvcl_triu_pearson_f32(const float* A, const float* B, int C, double* out6, void* workspace, size_t workspace_bytes, void* stream);
int cvcl_paired_l2_f32(const float* x, const float* y, int C, int D, float eps, float* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Word statistics (csrc/token_items.hip): the per-word language-model analysis of the reference's analysis_tools/processing.py.
 * Both entries validate everything before they enqueue anything (CVCL_EINVAL, cvcl_last_error names the argument), enqueue on the
 * caller's stream only and use no atomics: two calls on the same inputs give the same bits.
 *
 * cvcl_token_items_accumulate: `token_pos_items[key] += SumData(1, loss_.item(), outputs_, None)` for every token of a batch
 *   (processing.py:326-331) as one in-order segmented sum.  outputs [N, H] f32 and loss [N] f32 are the batch's N = B L positions;
 *   the positions that carry a key are listed by a CSR over the keys present in the batch: segment s covers rows[seg_ptr[s] ..
 *   seg_ptr[s + 1]) (int32 row indices in [0, N), ascending = the reference's visiting order; n_valid = seg_ptr[S]) and adds into
 *   entry slot[s] of the running tables vector [K, H] f32, loss_sum [K] double, cnt [K] int64.  One workgroup owns a (slot, column
 *   range): it loads the running value and adds the rows one by one, ((acc + v1) + v2) + ..., in fp32 for the vector and in double
 *   for the loss -- the reference's sums bit for bit, whatever H (no alignment requirement).  The slots of a call must be distinct.
 *   A segment whose slot lies outside [0, K) or whose bounds are not 0 <= begin < end <= n_valid is left out, and so is a row
 *   index outside [0, N): nothing is read or written out of bounds.  S = 0 is allowed (nothing happens).  CVCL_K_OTHER.
 * cvcl_token_topk: `logits.softmax(-1)` (processing.py:352) and `values.topk(top_k, -1)` (analysis_tools/utils.py:142) in one
 *   pass.  logits [R, V] f32, labels [R] int64, 1 <= k <= CVCL_TOKEN_TOPK_MAX_K, k <= V <= 12288 (a row is held in LDS and read
 *   from memory once) -> top_prob [R, k] f32 and top_idx [R, k] int64 ordered by (probability desc, index asc): ties go to the
 *   lower index; label_prob [R] f32 = the probability of labels[r], 0 where the label is pad_id or outside [0, V); probs [R, V]
 *   f32 = the whole softmax when the pointer is not NULL (nothing is written otherwise; it must not alias logits).  The logits
 *   must be finite, or -inf in some but not all entries of a row: a row of -inf only, or one holding +inf or NaN, has NaN
 *   probabilities and no order, and its top_idx entries are written as INT32_MAX (never used as an address).  CVCL_K_HEAD. */
enum { CVCL_TOKEN_TOPK_MAX_K = 16 };
int cvcl_token_items_accumulate(const float* outputs, const float* loss, int N, int H, const int32_t* seg_ptr, const int32_t* rows,
                                const int32_t* slot, int S, int n_valid, float* vector, double* loss_sum, int64_t* cnt, int K,
                                void* stream);
int cvcl_token_topk(const float* logits, const int64_t* labels, long R, int V, int k, int pad_id, float* top_prob, int64_t* top_idx,
                    float* label_prob, float* probs, void* stream);

/* ------------------------------------------------------------------------------------------
 * N-gram baseline (csrc/ngram.hip, ABI v7 additive): the back-off n-gram language model of the reference's top-level ngram.py,
 * which its analysis_tools/processing.py sets beside the LSTM.  All three entries validate everything before they enqueue anything
 * (CVCL_EINVAL, cvcl_last_error names the argument), enqueue ONE kernel on the caller's stream whatever N, and use no atomics:
 * two calls on the same inputs give the same bits.  CVCL_K_OTHER.
 *
 * Packing: bits = max(1, bit_length(vocab_size - 1)); an (n + 1)-gram is the big-endian concatenation of its token ids in a
 *   non-negative int64 -- the n context tokens in the high places, the predicted word in the low `bits` -- so the continuations
 *   of a context are one contiguous run of a sorted table.  1 <= N <= CVCL_NGRAM_MAX_N and N * bits <= 63 (vocab_size 2350: 12
 *   bits, N <= 5); bit 63 stays free: CVCL_NGRAM_SENTINEL is negative and sorts in front of every key.
 * y [B, L] int64 token ids (position 0 is <sos>: never predicted, but part of contexts), y_len [B] int64, clamped to [0, L] as the
 *   reference's slice y[b, :y_len[b]] does.  bad [1] int on the device receives the number of ids outside [0, vocab_size) found
 *   inside the utterance lengths (ids are read through the bit mask, so such an id cannot reach another key's bits; the caller
 *   decides what a non-zero count means).  B >= 0, L >= 1, B * L < 2^31.
 * cvcl_ngram_keys: ngram.py:28-36.  keys [N, B, L] int64: keys[n, b, i] = the packed gram y[b, i - n .. i] where
 *   max(1, n) <= i < len_b -- the (context, word) pairs NGramModel.update counts at order n -- and CVCL_NGRAM_SENTINEL elsewhere.
 *   Sorting a [n] slice and run-length counting it gives order n's table; a context's total is the sum over its run.
 * Tables (the next two entries): order n's grams are gram_key / gram_cnt [gram_off[n], gram_off[n + 1]) (device, int64, keys
 *   ascending and distinct), its contexts ctx_key (the gram keys >> bits) / ctx_tot [ctx_off[n], ctx_off[n + 1]).  gram_off and
 *   ctx_off are HOST arrays of N + 1 int64: they start at 0, do not decrease and end at n_gram / n_ctx; an order has contexts
 *   exactly when it has grams, no more contexts than grams, and order 0 at most one (the empty context, key 0).
 *   log_alpha = log(alpha), log_1m_alpha = log(1 - alpha), both <= 0.
 * cvcl_ngram_ce_loss: ngram.py:54-74 (calculate_ce_loss, tokenwise).  loss [B, L - 1] f32, fully written: loss[b, i - 1] =
 *   -logprob(b, i, y[b, i]) for 1 <= i < len_b, 0 elsewhere.  logprob walks n = min(N - 1, i) .. 0: at n >= 1, if the context
 *   y[b, i - n .. i) has been counted and the word seen after it, log c(ctx, w) - log c(ctx) + log_1m_alpha ends the walk; at
 *   n = 0, log(c(w) + 1) - log(total + vocab_size) ends it; every order left behind adds log_alpha.  Two lower-bound binary
 *   searches per step; log and the sum in double, in the reference's order of additions; one rounding to f32.  One thread per
 *   position.  With empty tables every scored position gets -(min(N - 1, i) + 1) log_alpha (the reference raises instead).
 * cvcl_ngram_probs: probs [B, L - 1, vocab_size] f32 = exp(logprob(b, i, w)) for EVERY candidate w, zero rows where the loss is 0;
 *   the same device function over a grid of (position, word).  B >= 1, L >= 2.  The values are the reference's back-off scores:
 *   they are NOT normalised over w (the mass alpha leaves for the lower orders is given to every word, seen or not).  The reference
 *   has no such output (its run_model(..., return_all=True) fails for an n-gram model). */
enum { CVCL_NGRAM_MAX_N = 8 };
#define CVCL_NGRAM_SENTINEL (-1)
int cvcl_ngram_keys(const int64_t* y, const int64_t* y_len, int B, int L, int N, int vocab_size, int64_t* keys, int* bad, void* stream);
int cvcl_ngram_ce_loss(const int64_t* gram_key, const int64_t* gram_cnt, const int64_t* gram_off, int64_t n_gram,
                       const int64_t* ctx_key, const int64_t* ctx_tot, const int64_t* ctx_off, int64_t n_ctx, int N, int vocab_size,
                       double log_alpha, double log_1m_alpha, const int64_t* y, const int64_t* y_len, int B, int L, float* loss,
                       int* bad, void* stream);
int cvcl_ngram_probs(const int64_t* gram_key, const int64_t* gram_cnt, const int64_t* gram_off, int64_t n_gram, const int64_t* ctx_key,
                     const int64_t* ctx_tot, const int64_t* ctx_off, int64_t n_ctx, int N, int vocab_size, double log_alpha,
                     double log_1m_alpha, const int64_t* y, const int64_t* y_len, int B, int L, float* probs, int* bad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Trial scores (csrc/trials.hip, ABI v7 additive): the scoring of the reference's forced-choice evaluation loop, eval.py:196-232 --
 * per trial `logits = model(img, label, label_len)`, `torch.softmax(logits, dim=-1)`, `torch.argmax(logits)` -- for ALL trials of an
 * evaluation at once, from features that were computed once per distinct frame and once per distinct word (multimodal/trials.py).
 *
 * cvcl_trial_scores: query [Nq, D] and cand [Nc, D] f32 rows, read in place through their leading dimensions ldq, ldc >= D (elements;
 *   no alignment beyond float).  q_idx [T] and c_idx [T, n] int32 (device) name the rows of trial t: its query row and its n
 *   candidate rows, 1 <= n <= CVCL_TRIAL_MAX_CHOICES.  log_scale: a device scalar (the model's logit_neg_log_temperature, CLIP's
 *   logit_scale) or NULL (= scale 1).
 *     logits[t][j] = expf(*log_scale) * <query[q_idx[t]], cand[c_idx[t][j]]>      [T, n] f32; the pointer may be NULL (not written)
 *     probs[t]     = softmax(logits[t]) in fp32, the maximum subtracted             [T, n] f32
 *     pred[t]      = the LOWEST j that attains the maximum logit                    [T] int32
 *   One kernel whatever T, a wave64 per trial, the query row's slice in registers, one reduction per candidate in an order that
 *   depends on D alone: a trial's bits do not depend on T, on its place in the table or on the grid.  No atomics, no workspace.
 *   Everything is validated before anything is enqueued (CVCL_EINVAL, cvcl_last_error names the argument): null query / cand /
 *   q_idx / c_idx / probs / pred, n outside 1 .. CVCL_TRIAL_MAX_CHOICES, D < 1, ldq or ldc < D, Nq or Nc < 1, T < 0.  T = 0
 *   enqueues nothing and succeeds.  The indices are device data and cannot be validated on the host: a trial with an index outside
 *   [0, Nq) / [0, Nc) reads no row at all and gets NaN logits, NaN probs and pred = -1; its neighbours are not affected.
 *   CVCL_K_HEAD. */
#define CVCL_TRIAL_MAX_CHOICES 16
int cvcl_trial_scores(const float* query, long ldq, int Nq, const float* cand, long ldc, int Nc, int D, const int32_t* q_idx,
                      const int32_t* c_idx, int T, int n, const float* log_scale, float* logits, float* probs, int32_t* pred,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Caption scores (csrc/textgen_scores.hip, ABI v7 additive): the n-gram arithmetic of the pycocoevalcap scorers that the reference's
 * multimodal/textgen_eval.py calls with default arguments -- BLEU-1..4 (option "closest"), ROUGE-L (beta 1.2) and CIDEr (n = 4,
 * sigma = 6) -- on sentences of integer ids; DESIGN.md "Caption scores" states the definitions.  All three entries validate
 * everything before they enqueue anything (CVCL_EINVAL, cvcl_last_error names the argument), enqueue ONE kernel on the caller's
 * stream, one workgroup per example, and use no atomics: two calls on the same inputs give the same bits.  Floating-point work is
 * in double.  CVCL_K_OTHER.
 *
 * Corpus: hyp [N, Lh] int64 ids in [0, vocab_size) with hyp_len [N] int64: the hypothesis of each of the N >= 1 examples.
 *   ref [R, Lr] int64 with ref_len [R]: every reference, example i owning the rows ref_off[i] .. ref_off[i + 1].  Lengths are
 *   clamped to [0, row width] as the n-gram entries clamp theirs; a length of 0 is an empty sentence.  ref_off is a HOST array of
 *   N + 1 int64 (it starts at 0, ends at R, and gives every example 1 .. CVCL_CAPTION_MAX_REFS rows); ref_off_dev is the caller's
 *   copy of the same values on the device, which the kernels read through clamps (a copy that differs gives wrong scores, never an
 *   access outside ref).  Limits: 1 <= Lh, Lr <= CVCL_CAPTION_MAX_LEN tokens per sentence, CVCL_CAPTION_ORDERS * bits <= 63 with
 *   bits = max(1, bit_length(vocab_size - 1)) (vocab_size <= 32768), N * Lh and R * Lr < 2^31.  Ids are read through the bit
 *   mask, as the n-gram entries read theirs.
 * cvcl_caption_bleu_rouge: stats [N, 10] int64 = testlen, the closest reflen (the reference length minimising (|l - testlen|, l)),
 *   guess[1..4] = max(0, testlen - n + 1), correct[1..4] = sum over the hypothesis' distinct n-grams of min(its count, the largest
 *   count in one reference); rouge [N] f64 = (1 + b^2) p r / (r + b^2 p), p = max_r LCS / len(hyp), r = max_r LCS / len(ref_r), each
 *   maximum on its own, 0 when either is 0 (an empty sentence contributes 0).  bad [1] int on the device receives the number of ids
 *   outside [0, vocab_size) inside the lengths of hyp and ref (the caller decides what a non-zero count means).
 * cvcl_caption_ref_keys: keys [CVCL_CAPTION_ORDERS, R, Lr] int64: keys[n - 1, r, q] = the packed n-gram ref[r, q .. q + n) (big-endian,
 *   `bits` per token, as "N-gram baseline" packs) where it fits the reference's length AND no earlier position of the same example's
 *   references holds it; CVCL_CAPTION_SENTINEL elsewhere.  Sorting slice n - 1 and run-length counting it gives order n's document
 *   frequencies: the number of examples whose references hold the n-gram.
 * cvcl_caption_cider: df_key / df_cnt [n_df] int64 on the device hold those tables, order n in [df_off[n - 1], df_off[n]) (keys
 *   ascending and distinct; df_off a HOST array of CVCL_CAPTION_ORDERS + 1 int64 from 0 to n_df).  cider [N] f64 = 10 * mean_n(sum_r
 *   sim_n(hyp, ref_r)) / n_refs with the vectors tf(g) * (log(N) - log(max(1, df(g)))) (df by binary search, 0 when absent), sim_n =
 *   sum_{g in hyp} min(h[g], r[g]) r[g] / (|h|_n |r|_n) (the division only when both norms are non-zero) times
 *   exp(-(len_h - len_r)^2 / (2 sigma^2)), a sentence's "length" being its number of bigram occurrences.  N = 1 gives 0. */
enum { CVCL_CAPTION_MAX_LEN = 128, CVCL_CAPTION_MAX_REFS = 32, CVCL_CAPTION_ORDERS = 4 };
#define CVCL_CAPTION_SENTINEL (-1)
int cvcl_caption_bleu_rouge(const int64_t* hyp, const int64_t* hyp_len, int N, int Lh, const int64_t* ref, const int64_t* ref_len, int R,
                            int Lr, const int64_t* ref_off, const int64_t* ref_off_dev, int vocab_size, int64_t* stats, double* rouge,
                            int* bad, void* stream);
int cvcl_caption_ref_keys(const int64_t* ref, const int64_t* ref_len, int N, int R, int Lr, const int64_t* ref_off,
                          const int64_t* ref_off_dev, int vocab_size, int64_t* keys, void* stream);
int cvcl_caption_cider(const int64_t* hyp, const int64_t* hyp_len, int N, int Lh, const int64_t* ref, const int64_t* ref_len, int R, int Lr,
                       const int64_t* ref_off, const int64_t* ref_off_dev, int vocab_size, const int64_t* df_key, const int64_t* df_cnt,
                       const int64_t* df_off, int64_t n_df, double* cider, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention overlays (csrc/overlay.hip, ABI v7 additive): what getAttMap / preprocess_attn_map (multimodal/attention_maps.py) do per
 * map on the host, for M maps in one call; DESIGN.md "Attention overlays" states the definitions.  Everything is validated before
 * anything is enqueued (CVCL_EINVAL, cvcl_last_error names the argument); the kernels run on the caller's stream only, in the caller's
 * workspace, without atomics: two calls give the same bits.  CVCL_K_OTHER.
 *   maps [M, h, w] f32; images [N, 3, H, W] f32 NCHW, normalised; mean, std: HOST arrays of 3 floats, the frame is img * std + mean
 *   (one multiply, one add); image_of_map [M] int32 on the device: the image under map m (NULL: image m, needs M <= N); lut [n_lut, 3]
 *   f32, 2 <= n_lut <= 1024.  Limits: 1 <= H, W <= 1024, 1 <= h <= H, 1 <= w <= W.  Per map, in order:
 *   1. (h, w) != (H, W): cvcl_bicubic_resize to H x W.
 *   2. CVCL_OVERLAY_BLUR: scipy.ndimage.gaussian_filter(map, sigma = 0.02 max(H, W)): separable, rows axis first, radius
 *      int(4 sigma + 0.5), weights exp(-t^2 / 2 sigma^2) normalised to sum 1 in double, mode "reflect" (period 2n, any radius), fp32 sums.
 *   3. x = (m - lo) / (hi - lo) with the map's own min / max (a constant map: x = m - lo = 0).  CVCL_OVERLAY_HAS_RANGE: lo = vmin,
 *      hi = vmax and x is clamped to [0, 1] (the host functions do not clamp, and their x ** 0.7 is NaN below vmin).
 *   4. colour = lut[min(int(x n_lut), n_lut - 1)];  5. t = x^gamma, out = (1 - t) frame + t colour  (0 <= gamma <= 64);
 *   6. out_u8 = floor(clamp(out, 0, 1) 255 + 0.5).
 *   CVCL_OVERLAY_IMAGE_ONLY: t = 0, out = frame; maps, lut, gamma, the range and out_map are not used (maps and lut may be NULL).
 *   Outputs, each optional, at least one: out_f32 / out_u8 hold pixel (y, x) channel c of map m at element dst_offset[m] + y row_pitch
 *   + 3 x + c (dst_offset [M] int64 on the device; NULL: m H row_pitch; row_pitch >= 3 W), so one launch writes the tiles of a larger
 *   canvas; out_elems is the element count of those buffers, and a map whose tile would not lie inside it (or whose image_of_map entry
 *   is outside [0, N)) is skipped.  out_map [M, H, W] f32: x.  NaN in a map: unspecified values, same accesses.
 *   maps, images, the outputs and the workspace are 16-byte aligned; workspace >= cvcl_attn_overlay_workspace_bytes (0 = refused sizes
 *   or flags, never 0 otherwise).                                                                                                  */
enum { CVCL_OVERLAY_BLUR = 1, CVCL_OVERLAY_HAS_RANGE = 2, CVCL_OVERLAY_IMAGE_ONLY = 4 };
size_t cvcl_attn_overlay_workspace_bytes(int M, int h, int w, int H, int W, int flags);
int cvcl_attn_overlay(const float* maps, int M, int h, int w, const float* images, int N, int H, int W, const float* mean,
                      const float* std, const int32_t* image_of_map, const float* lut, int n_lut, int flags, float gamma, float vmin,
                      float vmax, const int64_t* dst_offset, int64_t row_pitch, int64_t out_elems, float* out_f32, uint8_t* out_u8,
                      float* out_map, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Map faithfulness (csrc/faithfulness.hip, ABI v7 additive): the pieces of the deletion / insertion curves of an attention map
 * (Petsiuk et al., RISE, 2018; multimodal/map_faithfulness.py; DESIGN.md "Map faithfulness").  Everything is validated before anything
 * is enqueued (CVCL_EINVAL, cvcl_last_error names the argument, nothing is written); the kernels run on the caller's stream only and
 * use no global atomics: two calls give the same bits.  CVCL_K_OTHER.
 * cvcl_map_ranks: maps [M, HW] f32 -> ranks [M, HW] int32: ranks[m][p] = the position of pixel p when map m's pixels are ordered by
 *   value descending.  Values compare as floats (-0.0 == +0.0; subnormals order by value, nothing is flushed), ties go to the lower
 *   flat index: every map's ranks are a permutation of 0 .. HW - 1.  NaN is not supported (the ranks stay a permutation, in an
 *   unspecified order).  Limits: 1 <= HW <= 65536, M >= 1.  scratch: 16-byte aligned, >= cvcl_map_ranks_scratch_bytes(M, HW) bytes
 *   (0 = refused sizes): two (key, index) buffers of 6 bytes per pixel per map.  One workgroup per map.
 * cvcl_map_perturb: work item i writes out[i] [C, H, W] from m = item_map[i], n = image_of_map[m] (NULL: n = m, needs M <= N),
 *   k = item_count[i] in [0, H W]:  item_mode[i] == 0 (deletion): pixel p is baseline[n] where ranks[m][p] < k, else images[n];
 *   item_mode[i] == 1 (insertion): images[n] where ranks[m][p] < k, else baseline[n].  A select: the output has the inputs' bits.
 *   images, baseline [N, C, H, W] f32 (baseline NULL: zeros), ranks [M, H W] int32 and out [n_items, C, H, W] are on the device;
 *   image_of_map [M], item_map, item_count, item_mode [n_items] are HOST arrays: every entry is checked against N, M, H W and {0, 1}
 *   here, and the items travel to the kernel in its argument block, 256 per launch.  H W <= 65536; any H, W (rows need no alignment).
 * cvcl_gaussian_blur_f32: y = the separable k-tap filter w of x [planes, H, W], along the rows (x axis) first, then along the columns,
 *   with reflect padding that does not repeat the edge (torch's "reflect"), taps added in index order in fp32.  w: a HOST array of k
 *   floats; k odd, k <= 129, k / 2 < min(H, W).  scratch: planes H W floats on the device; x, y and scratch are distinct.
 * cvcl_pair_dot: out[r] = sum_e rows[r][e] targets[target_of_row[r]][e], rows [R, E], targets [M, E] f32, target_of_row [R] int32 on
 *   the device; a row whose index is outside [0, M) reads nothing and gets NaN.  One wave per row: lane l adds e = l, l + 64, ...
 * cvcl_curve_auc: auc[k][m] = sum_{s < S} (x[s + 1] - x[s]) (y[k][s][m] + y[k][s + 1][m]) / 2, y [K, S + 1, M], x [S + 1], auc [K, M]
 *   f32 on the device; S >= 1.                                                                                                     */
size_t cvcl_map_ranks_scratch_bytes(int M, int HW);
int cvcl_map_ranks(const float* maps, int32_t* ranks, int M, int HW, void* scratch, size_t scratch_bytes, void* stream);
int cvcl_map_perturb(const float* images, const float* baseline, const int32_t* ranks, const int32_t* image_of_map,
                     const int32_t* item_map, const int32_t* item_count, const int32_t* item_mode, int n_items, int N, int M, int C,
                     int H, int W, float* out, void* stream);
int cvcl_gaussian_blur_f32(const float* x, float* y, const float* w, int k, int planes, int H, int W, void* scratch, void* stream);
int cvcl_pair_dot(const float* rows, const float* targets, const int32_t* target_of_row, float* out, int R, int M, int E, void* stream);
int cvcl_curve_auc(const float* y, const float* x, float* auc, int K, int S, int M, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CVCL_HIP_H */
