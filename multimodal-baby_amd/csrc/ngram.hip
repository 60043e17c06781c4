// The back-off n-gram baseline of the word-level analysis (include/cvcl_hip.h "N-gram baseline"): the reference's top-level
// ngram.py.  cvcl_ngram_keys replaces the dict updates of NGramModel.update (ngram.py:28-36: one defaultdict lookup per token and
// order) by one packed key per (order, position) -- sorting and run-length counting them is the caller's plumbing;
// cvcl_ngram_ce_loss replaces the scoring loops of calculate_ce_loss (ngram.py:54-74); cvcl_ngram_probs scores every candidate word
// with the same chain (the reference has no such output).  All three are latency-bound: a few dependent binary searches per thread
// in tables that fit in L2.
#include "cvcl_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;

// The tables of all orders by value: order n's grams are gram_key / gram_cnt [gram_off[n], gram_off[n + 1]), its contexts
// ctx_key / ctx_tot [ctx_off[n], ctx_off[n + 1]); both sorted ascending, keys distinct and non-negative.
struct NgramTables {
    const int64_t* gram_key;
    const int64_t* gram_cnt;
    const int64_t* ctx_key;
    const int64_t* ctx_tot;
    int64_t gram_off[CVCL_NGRAM_MAX_N + 1];
    int64_t ctx_off[CVCL_NGRAM_MAX_N + 1];
    int N, bits, vocab_size;
    double log_alpha, log_1m_alpha;
};

// ngram.py:58-69, the back-off chain of position i of the utterance `history` for the candidate word w: from the longest order
// the position allows down to the unigram, log(alpha) per order left behind; the sum in double, in the reference's order of
// additions.  Tokens are read through the bit mask, so no id can reach the sign bit.
__device__ inline double ngram_logprob(const NgramTables& t, const int64_t* __restrict__ history, int i, int64_t w) {
    const int64_t mask = ((int64_t)1 << t.bits) - 1;
    const int top = min(t.N - 1, i);
    int64_t ctx_full = 0;                                  // history[i - top .. i), big-endian
    for (int j = i - top; j < i; ++j) ctx_full = (ctx_full << t.bits) | (history[j] & mask);
    w &= mask;
    double lp = 0.0;
    for (int n = top; n >= 0; --n) {
        const int64_t ctx = n ? (ctx_full & (((int64_t)1 << (n * t.bits)) - 1)) : 0;     // the last n tokens
        const int64_t c = cvcl_find_key(t.ctx_key, t.ctx_off[n], t.ctx_off[n + 1], ctx);
        if (c >= 0) {
            const int64_t g = cvcl_find_key(t.gram_key, t.gram_off[n], t.gram_off[n + 1], (ctx << t.bits) | w);
            if (n == 0) {
                const int64_t seen = g >= 0 ? t.gram_cnt[g] : 0;
                return lp + (log((double)(seen + 1)) - log((double)(t.ctx_tot[c] + t.vocab_size)));
            }
            if (g >= 0) return lp + ((log((double)t.gram_cnt[g]) - log((double)t.ctx_tot[c])) + t.log_1m_alpha);
        }
        lp += t.log_alpha;
    }
    return lp;                                             // nothing counted at all: the host refuses such a model
}

__device__ inline int ngram_len(const int64_t* __restrict__ y_len, int b, int L) {
    const int64_t n = y_len[b];
    return (int)(n < 0 ? 0 : (n > L ? L : n));             // y[b, :y_len[b]] of ngram.py:29 / :55 (lengths >= 0)
}

// Workgroup 0 alone counts the ids outside [0, vocab_size) inside the utterance lengths: one fixed-order sum, no atomics.
__device__ inline void ngram_count_bad(const int64_t* __restrict__ y, const int64_t* __restrict__ y_len, int B, int L,
                                       int vocab_size, int* __restrict__ bad) {
    __shared__ int s_bad[kThreads];
    int n = 0;
    for (long p = threadIdx.x; p < (long)B * L; p += kThreads) {
        const int b = (int)(p / L), i = (int)(p % L);
        const int64_t v = y[p];
        n += i < ngram_len(y_len, b, L) && (v < 0 || v >= vocab_size);
    }
    s_bad[threadIdx.x] = n;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_bad[threadIdx.x] += s_bad[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *bad = s_bad[0];
}

// One thread per position (b, i): the packed (n + 1)-gram that ends at i for every order n, or the sentinel where
// ngram.py:33 does not count (i < max(1, n) or i >= len).  keys is [N, B, L].
__global__ __launch_bounds__(kThreads) void ngram_keys_kernel(const int64_t* __restrict__ y, const int64_t* __restrict__ y_len, int B,
                                                              int L, int N, int bits, int vocab_size, int64_t* __restrict__ keys,
                                                              int* __restrict__ bad) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p < (long)B * L) {
        const int b = (int)(p / L), i = (int)(p % L);
        const int len = ngram_len(y_len, b, L);
        const int64_t mask = ((int64_t)1 << bits) - 1;
        const int64_t* s = y + (long)b * L;
        int64_t key = 0;
        for (int n = 0; n < N; ++n) {
            const bool counted = i < len && i >= max(1, n);
            if (counted) key |= (s[i - n] & mask) << (n * bits);         // token i - n sits n places above the predicted word
            keys[((long)n * B + b) * L + i] = counted ? key : (int64_t)CVCL_NGRAM_SENTINEL;
        }
    }
    if (blockIdx.x == 0) ngram_count_bad(y, y_len, B, L, vocab_size, bad);
}

// One thread per scored position (b, i), 1 <= i < L: loss[b, i - 1] = -ngram_logprob, 0 outside the utterance.
__global__ __launch_bounds__(kThreads) void ngram_ce_loss_kernel(NgramTables t, const int64_t* __restrict__ y,
                                                                 const int64_t* __restrict__ y_len, int B, int L,
                                                                 float* __restrict__ loss, int* __restrict__ bad) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p < (long)B * (L - 1)) {
        const int b = (int)(p / (L - 1)), i = (int)(p % (L - 1)) + 1;
        const int64_t* s = y + (long)b * L;
        loss[p] = i < ngram_len(y_len, b, L) ? (float)-ngram_logprob(t, s, i, s[i]) : 0.f;
    }
    if (blockIdx.x == 0) ngram_count_bad(y, y_len, B, L, t.vocab_size, bad);
}

// blockIdx.x: the position (b, i); blockIdx.y x 256 threads: the candidate words.  A workgroup shares its history, so its
// context searches branch uniformly -- and are repeated by every thread: up to N searches of ~18 dependent loads each that one
// lane per workgroup could do once and leave in LDS, with one gram search per word and order remaining.  Kept as it is so that
// the loss and the probabilities share ngram_logprob, one spelling; the whole [256, 24, 2350] grid takes 359 us at N = 3.
__global__ __launch_bounds__(kThreads) void ngram_probs_kernel(NgramTables t, const int64_t* __restrict__ y,
                                                               const int64_t* __restrict__ y_len, int B, int L,
                                                               float* __restrict__ probs, int* __restrict__ bad) {
    const long p = blockIdx.x;
    const int b = (int)(p / (L - 1)), i = (int)(p % (L - 1)) + 1;
    const int w = blockIdx.y * kThreads + threadIdx.x;
    if (w < t.vocab_size) {
        const bool inside = i < ngram_len(y_len, b, L);
        probs[p * t.vocab_size + w] = inside ? (float)exp(ngram_logprob(t, y + (long)b * L, i, w)) : 0.f;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) ngram_count_bad(y, y_len, B, L, t.vocab_size, bad);
}

// The checks the three entries share; -> bits through *bits.
int check_model(const char* entry, int N, int vocab_size, int B, int L, int* bits) {
    CVCL_CHECK_ARG(N >= 1 && N <= CVCL_NGRAM_MAX_N, "%s: N %d outside 1..%d", entry, N, CVCL_NGRAM_MAX_N);
    CVCL_CHECK_ARG(vocab_size >= 1, "%s: vocab_size %d < 1", entry, vocab_size);
    *bits = cvcl_key_bits(vocab_size);
    CVCL_CHECK_ARG(N * *bits <= 63, "%s: N %d x %d bits per token (vocab_size %d) > 63 key bits", entry, N, *bits, vocab_size);
    CVCL_CHECK_ARG(B >= 0, "%s: B %d < 0", entry, B);
    CVCL_CHECK_ARG(L >= 1, "%s: L %d < 1", entry, L);
    CVCL_CHECK_ARG((long)B * L < 0x7fffffffL, "%s: B %d x L %d positions do not fit 31 bits", entry, B, L);
    return CVCL_OK;
}

int check_tables(const char* entry, NgramTables* t, int N, int vocab_size, int bits, const int64_t* gram_key, const int64_t* gram_cnt,
                 const int64_t* gram_off, int64_t n_gram, const int64_t* ctx_key, const int64_t* ctx_tot, const int64_t* ctx_off,
                 int64_t n_ctx, double log_alpha, double log_1m_alpha) {
    CVCL_CHECK_ARG(gram_off && ctx_off, "%s: null pointer (gram_off / ctx_off)", entry);
    CVCL_CHECK_ARG(n_gram >= 0 && n_ctx >= 0, "%s: negative table size (n_gram %ld, n_ctx %ld)", entry, (long)n_gram, (long)n_ctx);
    CVCL_CHECK_ARG(gram_off[0] == 0 && gram_off[N] == n_gram, "%s: gram_off must run from 0 to n_gram %ld (got %ld .. %ld)", entry,
                   (long)n_gram, (long)gram_off[0], (long)gram_off[N]);
    CVCL_CHECK_ARG(ctx_off[0] == 0 && ctx_off[N] == n_ctx, "%s: ctx_off must run from 0 to n_ctx %ld (got %ld .. %ld)", entry,
                   (long)n_ctx, (long)ctx_off[0], (long)ctx_off[N]);
    for (int n = 0; n < N; ++n) {
        const int64_t g = gram_off[n + 1] - gram_off[n], c = ctx_off[n + 1] - ctx_off[n];
        CVCL_CHECK_ARG(g >= 0 && c >= 0, "%s: gram_off / ctx_off decrease at order %d", entry, n);
        CVCL_CHECK_ARG(c <= g && (c > 0) == (g > 0), "%s: order %d has %ld contexts for %ld grams (every context has a gram)", entry,
                       n, (long)c, (long)g);
        CVCL_CHECK_ARG(n > 0 || c <= 1, "%s: order 0 has %ld contexts (the empty context is the only one)", entry, (long)c);
    }
    CVCL_CHECK_ARG(n_gram == 0 || (gram_key && gram_cnt && ctx_key && ctx_tot),
                   "%s: null pointer (gram_key / gram_cnt / ctx_key / ctx_tot)", entry);
    CVCL_CHECK_ARG(log_alpha <= 0.0 && log_1m_alpha <= 0.0, "%s: log_alpha %g / log_1m_alpha %g is positive or NaN", entry, log_alpha,
                   log_1m_alpha);
    t->gram_key = gram_key; t->gram_cnt = gram_cnt; t->ctx_key = ctx_key; t->ctx_tot = ctx_tot;
    for (int n = 0; n <= CVCL_NGRAM_MAX_N; ++n) {
        t->gram_off[n] = gram_off[n < N ? n : N];
        t->ctx_off[n] = ctx_off[n < N ? n : N];
    }
    t->N = N; t->bits = bits; t->vocab_size = vocab_size; t->log_alpha = log_alpha; t->log_1m_alpha = log_1m_alpha;
    return CVCL_OK;
}

}  // namespace

extern "C" int cvcl_ngram_keys(const int64_t* y, const int64_t* y_len, int B, int L, int N, int vocab_size, int64_t* keys, int* bad,
                               void* stream) {
    int bits;
    if (int rc = check_model("cvcl_ngram_keys", N, vocab_size, B, L, &bits)) return rc;
    CVCL_CHECK_ARG(bad, "cvcl_ngram_keys: null pointer (bad)");
    CVCL_CHECK_ARG(B == 0 || (y && y_len && keys), "cvcl_ngram_keys: null pointer (y / y_len / keys)");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(ngram_keys_kernel, dim3(cvcl_div_up((long)B * L, kThreads) + (B == 0)), dim3(kThreads), 0, (hipStream_t)stream,
                       y, y_len, B, L, N, bits, vocab_size, keys, bad);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_ngram_ce_loss(const int64_t* gram_key, const int64_t* gram_cnt, const int64_t* gram_off, int64_t n_gram,
                                  const int64_t* ctx_key, const int64_t* ctx_tot, const int64_t* ctx_off, int64_t n_ctx, int N,
                                  int vocab_size, double log_alpha, double log_1m_alpha, const int64_t* y, const int64_t* y_len, int B,
                                  int L, float* loss, int* bad, void* stream) {
    int bits;
    NgramTables t;
    if (int rc = check_model("cvcl_ngram_ce_loss", N, vocab_size, B, L, &bits)) return rc;
    if (int rc = check_tables("cvcl_ngram_ce_loss", &t, N, vocab_size, bits, gram_key, gram_cnt, gram_off, n_gram, ctx_key, ctx_tot,
                              ctx_off, n_ctx, log_alpha, log_1m_alpha))
        return rc;
    CVCL_CHECK_ARG(bad, "cvcl_ngram_ce_loss: null pointer (bad)");
    CVCL_CHECK_ARG(B == 0 || (y && y_len), "cvcl_ngram_ce_loss: null pointer (y / y_len)");
    CVCL_CHECK_ARG(B == 0 || L == 1 || loss, "cvcl_ngram_ce_loss: null pointer (loss)");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    const long positions = (long)B * (L - 1);
    hipLaunchKernelGGL(ngram_ce_loss_kernel, dim3(cvcl_div_up(positions, kThreads) + (positions == 0)), dim3(kThreads), 0,
                       (hipStream_t)stream, t, y, y_len, B, L, loss, bad);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_ngram_probs(const int64_t* gram_key, const int64_t* gram_cnt, const int64_t* gram_off, int64_t n_gram,
                                const int64_t* ctx_key, const int64_t* ctx_tot, const int64_t* ctx_off, int64_t n_ctx, int N,
                                int vocab_size, double log_alpha, double log_1m_alpha, const int64_t* y, const int64_t* y_len, int B,
                                int L, float* probs, int* bad, void* stream) {
    int bits;
    NgramTables t;
    if (int rc = check_model("cvcl_ngram_probs", N, vocab_size, B, L, &bits)) return rc;
    if (int rc = check_tables("cvcl_ngram_probs", &t, N, vocab_size, bits, gram_key, gram_cnt, gram_off, n_gram, ctx_key, ctx_tot,
                              ctx_off, n_ctx, log_alpha, log_1m_alpha))
        return rc;
    CVCL_CHECK_ARG(cvcl_div_up(vocab_size, kThreads) <= 65535, "cvcl_ngram_probs: vocab_size %d is too large for one launch", vocab_size);
    CVCL_CHECK_ARG(bad, "cvcl_ngram_probs: null pointer (bad)");
    CVCL_CHECK_ARG(B >= 1 && L >= 2, "cvcl_ngram_probs: no position to score (B %d, L %d)", B, L);
    CVCL_CHECK_ARG(y && y_len && probs, "cvcl_ngram_probs: null pointer (y / y_len / probs)");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(ngram_probs_kernel, dim3((unsigned)((long)B * (L - 1)), cvcl_div_up(vocab_size, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, t, y, y_len, B, L, probs, bad);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
