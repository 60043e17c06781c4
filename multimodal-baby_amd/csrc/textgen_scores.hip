// Caption scores (include/cvcl_hip.h "Caption scores"): the n-gram arithmetic of the three pycocoevalcap scorers the reference's
// multimodal/textgen_eval.py calls that need nothing but token counts -- BLEU-1..4 (bleu_scorer.py, option "closest"), ROUGE-L
// (rouge.py, beta 1.2) and CIDEr (cider_scorer.py, n = 4, sigma = 6) -- on sentences of integer ids.  One workgroup per example:
// the example's sentences lie in LDS as one packed 4-gram per position, an n-gram is the top n tokens of that key, and counting an
// n-gram in a sentence is a scan of its positions (a caption has ~12 tokens, an example ~5 references: a few thousand compares and
// no table).  No atomics; every floating-point sum is in double, by one thread, in the package's order of additions.
#include "cvcl_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLen = CVCL_CAPTION_MAX_LEN;
constexpr int kMaxRefs = CVCL_CAPTION_MAX_REFS;
constexpr int kOrders = CVCL_CAPTION_ORDERS;

// The corpus as every kernel reads it.  ref_off is the DEVICE copy of the offsets the entry validated on the host; it is read
// through clamps (example_refs), so whatever it holds no row outside ref [R, Lr] is touched.
struct Corpus {
    const int64_t* hyp; const int64_t* hyp_len;
    const int64_t* ref; const int64_t* ref_len; const int64_t* ref_off;
    int N, Lh, R, Lr, bits, vocab_size;
};

// order n's table is key / cnt [off[n - 1], off[n]): the packed n-grams of the references, ascending and distinct, and the number
// of examples whose references hold each
struct DfTables {
    const int64_t* key; const int64_t* cnt;
    int64_t off[kOrders + 1];
};

// One example in LDS.  key[q] packs the tokens q .. q + 3 of a sentence big-endian, zeros past its end: its n-gram at q (q + n <=
// len) is key[q] >> ((4 - n) * bits), which is also that n-gram's packed key of the df tables.  Reference r's row starts at r * Lr.
struct Example {
    int64_t hyp_key[kMaxLen];
    int64_t ref_key[kMaxRefs * kMaxLen];
    int ref_len[kMaxRefs];
};

__device__ inline int caption_len(const int64_t* __restrict__ len, long row, int L) {
    const int64_t n = len[row];
    return (int)(n < 0 ? 0 : (n > L ? L : n));
}

__device__ inline int64_t key4_at(const int64_t* __restrict__ s, int q, int len, int bits) {
    const int64_t mask = ((int64_t)1 << bits) - 1;             // ids are read through the mask: none reaches another token's bits
    int64_t k = 0;
    for (int j = 0; j < kOrders; ++j) k = (k << bits) | (q + j < len ? (s[q + j] & mask) : 0);
    return k;
}

// -> the first reference row of example i; *n_refs in 0 .. kMaxRefs, the rows inside [0, R)
__device__ inline int example_refs(const Corpus& c, int i, int* n_refs) {
    const int64_t a = c.ref_off[i], b = c.ref_off[i + 1];
    const int r0 = (int)(a < 0 ? 0 : (a > c.R ? c.R : a));
    const int64_t top = min((int64_t)c.R, (int64_t)r0 + kMaxRefs);
    *n_refs = (int)(b < r0 ? 0 : (b > top ? top : b) - r0);
    return r0;
}

// Fills `e` with example i (the hypothesis only when the corpus has one); -> its hypothesis length.  Ends with a barrier.
__device__ inline int load_example(Example& e, const Corpus& c, int i, int r0, int n_refs) {
    const int hl = c.hyp ? caption_len(c.hyp_len, i, c.Lh) : 0;
    for (int p = threadIdx.x; p < hl; p += kThreads) e.hyp_key[p] = key4_at(c.hyp + (long)i * c.Lh, p, hl, c.bits);
    for (int f = threadIdx.x; f < n_refs * c.Lr; f += kThreads) {
        const int r = f / c.Lr, q = f % c.Lr;
        const int rl = caption_len(c.ref_len, r0 + r, c.Lr);
        if (q == 0) e.ref_len[r] = rl;
        e.ref_key[f] = key4_at(c.ref + (long)(r0 + r) * c.Lr, q, rl, c.bits);
    }
    __syncthreads();
    return hl;
}

// occurrences of the n-gram g among the positions [from, len - n] of a sentence whose keys start at `key`
__device__ inline int count_gram(const int64_t* key, int from, int len, int n, int shift, int64_t g) {
    int c = 0;
    for (int q = from; q + n <= len; ++q) c += (key[q] >> shift) == g;
    return c;
}

// the ids outside [0, vocab_size) inside the lengths of the rows of s [rows, L], by this thread's share of the positions
__device__ inline int bad_ids(const int64_t* __restrict__ s, const int64_t* __restrict__ len, int rows, int L, int vocab_size) {
    int n = 0;
    for (long p = threadIdx.x; p < (long)rows * L; p += kThreads) {
        const int64_t v = s[p];
        n += (int)(p % L) < caption_len(len, p / L, L) && (v < 0 || v >= vocab_size);
    }
    return n;
}

// bleu_scorer.py cook_refs / cook_test and rouge.py calc_score for example blockIdx.x.  stats[i] = testlen, the closest reflen,
// guess[1..4], correct[1..4].
__global__ __launch_bounds__(kThreads) void caption_bleu_rouge_kernel(Corpus c, int64_t* __restrict__ stats, double* __restrict__ rouge,
                                                                      int* __restrict__ bad) {
    __shared__ Example e;
    __shared__ int s_clip[kOrders * kMaxLen];                  // min(count in the hypothesis, max over references) per (n, p)
    __shared__ unsigned char s_row[kMaxRefs][kMaxLen + 1];     // the rolling row of each reference's LCS table (values <= 128)
    __shared__ int s_lcs[kMaxRefs];
    __shared__ int s_bad[kThreads];
    const int i = blockIdx.x;
    int n_refs;
    const int r0 = example_refs(c, i, &n_refs);
    const int hl = load_example(e, c, i, r0, n_refs);
    const int tok_shift = (kOrders - 1) * c.bits;

    // rouge.py my_lcs: one thread per reference walks the classic table, the hypothesis along the row
    if ((int)threadIdx.x < n_refs) {
        unsigned char* row = s_row[threadIdx.x];
        const int64_t* rk = e.ref_key + threadIdx.x * c.Lr;
        for (int j = 0; j <= hl; ++j) row[j] = 0;
        for (int q = 0; q < e.ref_len[threadIdx.x]; ++q) {
            const int64_t tok = rk[q] >> tok_shift;
            int diag = 0;
            for (int j = 1; j <= hl; ++j) {
                const int up = row[j];
                row[j] = (unsigned char)((e.hyp_key[j - 1] >> tok_shift) == tok ? diag + 1 : max(up, (int)row[j - 1]));
                diag = up;
            }
        }
        s_lcs[threadIdx.x] = row[hl];
    }
    // the clipped count of every n-gram of the hypothesis, at its first occurrence
    for (int item = threadIdx.x; item < kOrders * hl; item += kThreads) {
        const int n = item / hl + 1, p = item % hl, shift = (kOrders - n) * c.bits;
        const int64_t g = e.hyp_key[p] >> shift;
        int clip = 0;
        if (p + n <= hl && count_gram(e.hyp_key, 0, p + n - 1, n, shift, g) == 0) {
            const int in_hyp = count_gram(e.hyp_key, p, hl, n, shift, g);
            int in_ref = 0;
            for (int r = 0; r < n_refs; ++r) in_ref = max(in_ref, count_gram(e.ref_key + r * c.Lr, 0, e.ref_len[r], n, shift, g));
            clip = min(in_hyp, in_ref);
        }
        s_clip[item] = clip;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int reflen = 0, best = -1;
        double pmax = 0.0, rmax = 0.0;
        for (int r = 0; r < n_refs; ++r) {
            const int rl = e.ref_len[r], d = abs(rl - hl);
            if (best < 0 || d < best || (d == best && rl < reflen)) { best = d; reflen = rl; }     // min over (|l - testlen|, l)
            if (hl > 0) pmax = fmax(pmax, s_lcs[r] / (double)hl);
            if (rl > 0) rmax = fmax(rmax, s_lcs[r] / (double)rl);
        }
        int64_t* st = stats + (long)i * 10;
        st[0] = hl;
        st[1] = reflen;
        for (int n = 1; n <= kOrders; ++n) {
            int correct = 0;
            for (int p = 0; p < hl; ++p) correct += s_clip[(n - 1) * hl + p];
            st[1 + n] = max(0, hl - n + 1);
            st[1 + kOrders + n] = correct;
        }
        const double beta2 = 1.2 * 1.2;
        rouge[i] = (pmax != 0.0 && rmax != 0.0) ? ((1.0 + beta2) * pmax * rmax) / (rmax + beta2 * pmax) : 0.0;
    }
    if (i == 0) {                                              // workgroup 0 alone counts the bad ids: one fixed-order sum
        __syncthreads();
        s_bad[threadIdx.x] = bad_ids(c.hyp, c.hyp_len, c.N, c.Lh, c.vocab_size) + bad_ids(c.ref, c.ref_len, c.R, c.Lr, c.vocab_size);
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_bad[threadIdx.x] += s_bad[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) *bad = s_bad[0];
    }
}

// cider_scorer.py compute_doc_freq: an n-gram counts once per example whose references hold it.  One thread per reference position
// compares it with every earlier position of the example's references, all four orders in one pass; keys is [4, R, Lr].
__global__ __launch_bounds__(kThreads) void caption_ref_keys_kernel(Corpus c, int64_t* __restrict__ keys) {
    __shared__ Example e;
    int n_refs;
    const int r0 = example_refs(c, blockIdx.x, &n_refs);
    load_example(e, c, blockIdx.x, r0, n_refs);
    for (int f = threadIdx.x; f < n_refs * c.Lr; f += kThreads) {
        const int r = f / c.Lr, q = f % c.Lr;
        const int64_t k = e.ref_key[f];
        unsigned seen = 0;                                     // bit n - 1: an earlier position holds this n-gram
        for (int r2 = 0; r2 <= r; ++r2) {
            const int64_t* rk = e.ref_key + r2 * c.Lr;
            const int len2 = e.ref_len[r2], end = r2 < r ? len2 : q;
            for (int q2 = 0; q2 < end; ++q2) {
                const int64_t x = rk[q2] ^ k;
                for (int n = 1; n <= kOrders; ++n) seen |= (unsigned)(q2 + n <= len2 && (x >> ((kOrders - n) * c.bits)) == 0) << (n - 1);
            }
        }
        for (int n = 1; n <= kOrders; ++n) {
            const bool first = q + n <= e.ref_len[r] && !((seen >> (n - 1)) & 1);
            keys[((long)(n - 1) * c.R + r0 + r) * c.Lr + q] = first ? k >> ((kOrders - n) * c.bits) : (int64_t)CVCL_CAPTION_SENTINEL;
        }
    }
}

// cider_scorer.py counts2vec: ref_len - log(max(1, df)) of the n-gram g, df = 0 for an n-gram no reference holds
__device__ inline double idf_weight(const DfTables& t, int n, int64_t g, double log_N) {
    const int64_t at = cvcl_find_key(t.key, t.off[n - 1], t.off[n], g);
    return log_N - (at >= 0 ? log(fmax(1.0, (double)t.cnt[at])) : 0.0);
}

// cider_scorer.py counts2vec / sim / compute_cider for example blockIdx.x
__global__ __launch_bounds__(kThreads) void caption_cider_kernel(Corpus c, DfTables t, double log_N, double* __restrict__ cider) {
    __shared__ Example e;
    __shared__ double s_hvec[kOrders * kMaxLen];               // tf x weight of the hypothesis n-gram first seen at (n, p), else 0
    __shared__ double s_wt[kOrders * kMaxLen];
    __shared__ double s_val[kMaxRefs][kOrders], s_norm2[kMaxRefs][kOrders];
    const int i = blockIdx.x;
    int n_refs;
    const int r0 = example_refs(c, i, &n_refs);
    const int hl = load_example(e, c, i, r0, n_refs);

    for (int item = threadIdx.x; item < kOrders * hl; item += kThreads) {
        const int n = item / hl + 1, p = item % hl, shift = (kOrders - n) * c.bits;
        const int64_t g = e.hyp_key[p] >> shift;
        double w = 0.0, v = 0.0;
        if (p + n <= hl && count_gram(e.hyp_key, 0, p + n - 1, n, shift, g) == 0) {
            w = idf_weight(t, n, g, log_N);
            v = (double)count_gram(e.hyp_key, p, hl, n, shift, g) * w;
        }
        s_wt[item] = w;
        s_hvec[item] = v;
    }
    __syncthreads();
    // one thread per (reference, order): the reference's squared norm and its product with the hypothesis, position by position
    if ((int)threadIdx.x < n_refs * kOrders) {
        const int r = threadIdx.x / kOrders, n = threadIdx.x % kOrders + 1, shift = (kOrders - n) * c.bits;
        const int64_t* rk = e.ref_key + r * c.Lr;
        const int rl = e.ref_len[r];
        double norm2 = 0.0, val = 0.0;
        for (int q = 0; q + n <= rl; ++q) {
            const int64_t g = rk[q] >> shift;
            if (count_gram(rk, 0, q + n - 1, n, shift, g)) continue;
            const double v = (double)count_gram(rk, q, rl, n, shift, g) * idf_weight(t, n, g, log_N);
            norm2 += v * v;
        }
        for (int p = 0; p + n <= hl; ++p) {
            const double hv = s_hvec[(n - 1) * hl + p];
            if (hv == 0.0) continue;                           // not a first occurrence, or weight 0: min(0, .) x . adds nothing
            const double rv = (double)count_gram(rk, 0, rl, n, shift, e.hyp_key[p] >> shift) * s_wt[(n - 1) * hl + p];
            val += fmin(hv, rv) * rv;
        }
        s_norm2[r][n - 1] = norm2;
        s_val[r][n - 1] = val;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double norm_h[kOrders], score[kOrders];
        for (int n = 0; n < kOrders; ++n) {
            double s = 0.0;
            for (int p = 0; p < hl; ++p) s += s_hvec[n * hl + p] * s_hvec[n * hl + p];
            norm_h[n] = sqrt(s);
            score[n] = 0.0;
        }
        const double sigma = 6.0;
        for (int r = 0; r < n_refs; ++r) {
            const double delta = (double)(max(0, hl - 1) - max(0, e.ref_len[r] - 1));      // "length": the bigram occurrences
            const double gauss = exp(-(delta * delta) / (2.0 * sigma * sigma));
            for (int n = 0; n < kOrders; ++n) {
                double v = s_val[r][n];
                const double norm_r = sqrt(s_norm2[r][n]);
                if (norm_h[n] != 0.0 && norm_r != 0.0) v /= norm_h[n] * norm_r;
                score[n] += v * gauss;
            }
        }
        const double mean = (((score[0] + score[1]) + score[2]) + score[3]) / kOrders;
        cider[i] = n_refs ? mean / n_refs * 10.0 : 0.0;
    }
}

// The checks the three entries share; fills the corpus but its hypothesis side.
int check_corpus(const char* entry, Corpus* c, int N, const int64_t* ref, const int64_t* ref_len, int R, int Lr, const int64_t* ref_off,
                 const int64_t* ref_off_dev, int vocab_size) {
    CVCL_CHECK_ARG(N >= 1, "%s: N %d < 1 (no example to score)", entry, N);
    CVCL_CHECK_ARG(vocab_size >= 1, "%s: vocab_size %d < 1", entry, vocab_size);
    const int bits = cvcl_key_bits(vocab_size);
    CVCL_CHECK_ARG(kOrders * bits <= 63, "%s: %d x %d bits per token (vocab_size %d) > 63 key bits", entry, kOrders, bits, vocab_size);
    CVCL_CHECK_ARG(Lr >= 1 && Lr <= kMaxLen, "%s: Lr %d outside 1..%d tokens per sentence", entry, Lr, kMaxLen);
    CVCL_CHECK_ARG(R >= 1 && (long)R * Lr < 0x7fffffffL, "%s: R %d references (x Lr %d) outside 1 .. 2^31 positions", entry, R, Lr);
    CVCL_CHECK_ARG(ref && ref_len && ref_off && ref_off_dev, "%s: null pointer (ref / ref_len / ref_off / ref_off_dev)", entry);
    CVCL_CHECK_ARG(ref_off[0] == 0 && ref_off[N] == R, "%s: ref_off must run from 0 to R %d (got %ld .. %ld)", entry, R, (long)ref_off[0],
                   (long)ref_off[N]);
    for (int i = 0; i < N; ++i) {
        const int64_t n = ref_off[i + 1] - ref_off[i];
        CVCL_CHECK_ARG(n >= 0, "%s: ref_off decreases at example %d", entry, i);
        CVCL_CHECK_ARG(n >= 1 && n <= kMaxRefs, "%s: example %d has %ld references (outside 1..%d)", entry, i, (long)n, kMaxRefs);
    }
    *c = Corpus{nullptr, nullptr, ref, ref_len, ref_off_dev, N, 0, R, Lr, bits, vocab_size};
    return CVCL_OK;
}

int check_hyp(const char* entry, Corpus* c, const int64_t* hyp, const int64_t* hyp_len, int Lh) {
    CVCL_CHECK_ARG(Lh >= 1 && Lh <= kMaxLen, "%s: Lh %d outside 1..%d tokens per sentence", entry, Lh, kMaxLen);
    CVCL_CHECK_ARG((long)c->N * Lh < 0x7fffffffL, "%s: N %d x Lh %d positions do not fit 31 bits", entry, c->N, Lh);
    CVCL_CHECK_ARG(hyp && hyp_len, "%s: null pointer (hyp / hyp_len)", entry);
    c->hyp = hyp; c->hyp_len = hyp_len; c->Lh = Lh;
    return CVCL_OK;
}

}  // namespace

extern "C" int cvcl_caption_bleu_rouge(const int64_t* hyp, const int64_t* hyp_len, int N, int Lh, const int64_t* ref,
                                       const int64_t* ref_len, int R, int Lr, const int64_t* ref_off, const int64_t* ref_off_dev,
                                       int vocab_size, int64_t* stats, double* rouge, int* bad, void* stream) {
    Corpus c;
    if (int rc = check_corpus("cvcl_caption_bleu_rouge", &c, N, ref, ref_len, R, Lr, ref_off, ref_off_dev, vocab_size)) return rc;
    if (int rc = check_hyp("cvcl_caption_bleu_rouge", &c, hyp, hyp_len, Lh)) return rc;
    CVCL_CHECK_ARG(stats && rouge && bad, "cvcl_caption_bleu_rouge: null pointer (stats / rouge / bad)");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(caption_bleu_rouge_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, c, stats, rouge, bad);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_caption_ref_keys(const int64_t* ref, const int64_t* ref_len, int N, int R, int Lr, const int64_t* ref_off,
                                     const int64_t* ref_off_dev, int vocab_size, int64_t* keys, void* stream) {
    Corpus c;
    if (int rc = check_corpus("cvcl_caption_ref_keys", &c, N, ref, ref_len, R, Lr, ref_off, ref_off_dev, vocab_size)) return rc;
    CVCL_CHECK_ARG(keys, "cvcl_caption_ref_keys: null pointer (keys)");
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(caption_ref_keys_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, c, keys);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}

extern "C" int cvcl_caption_cider(const int64_t* hyp, const int64_t* hyp_len, int N, int Lh, const int64_t* ref, const int64_t* ref_len,
                                  int R, int Lr, const int64_t* ref_off, const int64_t* ref_off_dev, int vocab_size,
                                  const int64_t* df_key, const int64_t* df_cnt, const int64_t* df_off, int64_t n_df, double* cider,
                                  void* stream) {
    Corpus c;
    DfTables t;
    if (int rc = check_corpus("cvcl_caption_cider", &c, N, ref, ref_len, R, Lr, ref_off, ref_off_dev, vocab_size)) return rc;
    if (int rc = check_hyp("cvcl_caption_cider", &c, hyp, hyp_len, Lh)) return rc;
    CVCL_CHECK_ARG(df_off, "cvcl_caption_cider: null pointer (df_off)");
    CVCL_CHECK_ARG(n_df >= 0 && df_off[0] == 0 && df_off[kOrders] == n_df, "cvcl_caption_cider: df_off must run from 0 to n_df %ld (got %ld .. %ld)",
                   (long)n_df, (long)df_off[0], (long)df_off[kOrders]);
    for (int n = 0; n < kOrders; ++n) CVCL_CHECK_ARG(df_off[n + 1] >= df_off[n], "cvcl_caption_cider: df_off decreases at order %d", n + 1);
    CVCL_CHECK_ARG(n_df == 0 || (df_key && df_cnt), "cvcl_caption_cider: null pointer (df_key / df_cnt)");
    CVCL_CHECK_ARG(cider, "cvcl_caption_cider: null pointer (cider)");
    t.key = df_key; t.cnt = df_cnt;
    for (int n = 0; n <= kOrders; ++n) t.off[n] = df_off[n];
    CvclProfScope prof(stream, CVCL_K_OTHER);
    hipLaunchKernelGGL(caption_cider_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, c, t, log((double)N), cider);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
