// Word-level language-model statistics (include/cvcl_hip.h "Word statistics"): the reduction by (word, tag) key of the reference's
// get_model_items (analysis_tools/processing.py:326-331: one .item() and one SumData.__add__ per token) and the softmax + top-k of
// its prediction listings (processing.py:352, analysis_tools/utils.py:142), both on the device.  Both kernels are memory-bound.
#include "cvcl_common.h"

#include <math.h>

namespace {

constexpr int kAccThreads = 256;                       // one column of the key's vector per thread
constexpr int kAccBatch = 8;                           // rows in flight per wait; the additions stay in row order

// One workgroup per (segment, 256-column range).  acc starts from the running value and takes the segment's rows one by one in
// `rows` order: ((acc + v1) + v2) + ... in fp32 -- the sum the reference's `token_pos_items[key] += sdata` forms.  The workgroup of
// column range 0 also owns the key's loss (float64, the same order) and count.  Nothing else touches the key's entries: no atomics.
__global__ __launch_bounds__(kAccThreads) void token_items_accumulate_kernel(
    const float* __restrict__ outputs, const float* __restrict__ loss, int N, int H, const int32_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ slot, int n_valid, int K, float* __restrict__ vector,
    double* __restrict__ loss_sum, int64_t* __restrict__ cnt) {
    const int s = blockIdx.x;
    const int k = slot[s];
    int r0 = seg_ptr[s], r1 = seg_ptr[s + 1];
    if ((unsigned)k >= (unsigned)K || r0 < 0 || r1 > n_valid || r0 >= r1) return;      // a malformed segment is left out whole
    const int col = blockIdx.y * kAccThreads + threadIdx.x;
    if (col < H) {
        float acc = vector[(long)k * H + col];
        for (int i0 = r0; i0 < r1; i0 += kAccBatch) {
            float v[kAccBatch];
            bool ok[kAccBatch];
#pragma unroll
            for (int u = 0; u < kAccBatch; ++u) {
                const int row = rows[min(i0 + u, r1 - 1)];
                ok[u] = i0 + u < r1 && (unsigned)row < (unsigned)N;
                v[u] = ok[u] ? outputs[(long)row * H + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kAccBatch; ++u)
                if (ok[u]) acc += v[u];
        }
        vector[(long)k * H + col] = acc;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        double acc = loss_sum[k];
        int64_t n = 0;
        for (int i0 = r0; i0 < r1; i0 += kAccBatch) {
            float v[kAccBatch];
            bool ok[kAccBatch];
#pragma unroll
            for (int u = 0; u < kAccBatch; ++u) {
                const int row = rows[min(i0 + u, r1 - 1)];
                ok[u] = i0 + u < r1 && (unsigned)row < (unsigned)N;
                v[u] = ok[u] ? loss[row] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kAccBatch; ++u)
                if (ok[u]) { acc += (double)v[u]; ++n; }
        }
        loss_sum[k] = acc;
        cnt[k] += n;
    }
}

constexpr int kTopThreads = 256;
constexpr int kTopWaves = kTopThreads / CVCL_WAVE;
constexpr int kTopMaxV = 12288;                        // the row lives in LDS: 48 KiB of the 64 KiB a workgroup gets by default

// One workgroup per row: the row is read once into LDS, turned into probabilities there, and the k best are taken in k rounds of a
// workgroup arg-max over (probability desc, index asc); round r looks only at the entries behind round r - 1's winner in that
// order, so nothing is erased and equal probabilities come out in index order.
__global__ __launch_bounds__(kTopThreads) void token_topk_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                 int V, int k, int pad_id, float* __restrict__ top_prob,
                                                                 int64_t* __restrict__ top_idx, float* __restrict__ label_prob,
                                                                 float* __restrict__ probs) {
    extern __shared__ float s_p[];                     // [V]
    __shared__ float s_red[kTopWaves];
    __shared__ float s_bs[2][kTopWaves];
    __shared__ int s_bi[2][kTopWaves];
    const long r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = logits + r * V;

    float m = -INFINITY;
    for (int v = tid; v < V; v += kTopThreads) {
        const float x = row[v];
        s_p[v] = x;
        m = fmaxf(m, x);
    }
    m = block_max(m, s_red);
    const float mm = isinf(m) ? 0.f : m;
    float sum = 0.f;
    for (int v = tid; v < V; v += kTopThreads) {       // every thread revisits the entries it wrote itself
        const float e = expf(s_p[v] - mm);
        s_p[v] = e;
        sum += e;
    }
    sum = block_sum(sum, s_red);
    for (int v = tid; v < V; v += kTopThreads) {
        const float p = s_p[v] / sum;
        s_p[v] = p;
        if (probs) stream_store(p, probs + r * V + v);
    }
    __syncthreads();
    if (tid == 0) {
        const int64_t lab = labels[r];
        label_prob[r] = (lab != pad_id && lab >= 0 && lab < V) ? s_p[lab] : 0.f;
    }

    float ps = INFINITY;                               // the previous round's winner: everything is behind (+inf, -1)
    int pi = -1;
    for (int round = 0; round < k; ++round) {
        float bs = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = tid; v < V; v += kTopThreads) {
            const float p = s_p[v];
            if (cvcl_better(ps, pi, p, v) && cvcl_better(p, v, bs, bi)) { bs = p; bi = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (cvcl_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { s_bs[round & 1][w] = bs; s_bi[round & 1][w] = bi; }
        __syncthreads();
        bs = s_bs[round & 1][0];
        bi = s_bi[round & 1][0];
#pragma unroll
        for (int q = 1; q < kTopWaves; ++q)
            if (cvcl_better(s_bs[round & 1][q], s_bi[round & 1][q], bs, bi)) { bs = s_bs[round & 1][q]; bi = s_bi[round & 1][q]; }
        if (tid == 0) {
            top_prob[r * k + round] = bs;
            top_idx[r * k + round] = bi;
        }
        ps = bs;
        pi = bi;
    }
}

}  // namespace

extern "C" int cvcl_token_items_accumulate(const float* outputs, const float* loss, int N, int H, const int32_t* seg_ptr,
                                           const int32_t* rows, const int32_t* slot, int S, int n_valid, float* vector,
                                           double* loss_sum, int64_t* cnt, int K, void* stream) {
    CVCL_CHECK_ARG(N >= 1 && H >= 1 && K >= 1 && S >= 0 && n_valid >= 0,
                   "cvcl_token_items_accumulate: bad sizes (N %d, H %d, K %d, S %d, n_valid %d)", N, H, K, S, n_valid);
    CVCL_CHECK_ARG(S <= K, "cvcl_token_items_accumulate: %d segments for %d keys (one segment per key at most)", S, K);
    if (S == 0) return CVCL_OK;                        // an empty batch: nothing to add
    CVCL_CHECK_ARG(n_valid >= S, "cvcl_token_items_accumulate: %d rows for %d segments (no segment is empty)", n_valid, S);
    CVCL_CHECK_ARG(outputs && loss && seg_ptr && rows && slot && vector && loss_sum && cnt, "cvcl_token_items_accumulate: null pointer");
    const int col_blocks = cvcl_div_up(H, kAccThreads);
    CVCL_CHECK_ARG(col_blocks <= 65535, "cvcl_token_items_accumulate: H %d is too wide", H);
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(token_items_accumulate_kernel, dim3(S, col_blocks), dim3(kAccThreads), 0, (hipStream_t)stream, outputs, loss, N,
                       H, seg_ptr, rows, slot, n_valid, K, vector, loss_sum, cnt);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_token_topk(const float* logits, const int64_t* labels, long R, int V, int k, int pad_id, float* top_prob,
                               int64_t* top_idx, float* label_prob, float* probs, void* stream) {
    CVCL_CHECK_ARG(k >= 1 && k <= CVCL_TOKEN_TOPK_MAX_K, "cvcl_token_topk: k %d outside [1, %d]", k, CVCL_TOKEN_TOPK_MAX_K);
    CVCL_CHECK_ARG(V >= k && V <= kTopMaxV, "cvcl_token_topk: vocabulary size %d outside [k = %d, %d]", V, k, kTopMaxV);
    CVCL_CHECK_ARG(R >= 1 && R < 0x7fffffffL, "cvcl_token_topk: bad row count %ld", R);
    CVCL_CHECK_ARG(logits && labels && top_prob && top_idx && label_prob, "cvcl_token_topk: null pointer");
    CVCL_CHECK_ARG(probs != logits, "cvcl_token_topk: probs must not alias logits");
    CvclProfScope prof(stream, CVCL_K_HEAD);
    hipLaunchKernelGGL(token_topk_kernel, dim3((unsigned)R), dim3(kTopThreads), (size_t)V * sizeof(float), (hipStream_t)stream, logits,
                       labels, V, k, pad_id, top_prob, top_idx, label_prob, probs);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
