// The discard_ratio variant of the ViT attention rollout (Gildenblat's vit-explain): before the chain, the k weakest attentions of
// every head-fused matrix are set to zero.
//
//   cvcl_attention_discard   F [n_mats][T][T] fp32 (cvcl_attention_head_fuse, csrc/vit_maps.hip), in place.  Per matrix, flattened
//                            row-major to M = T T elements: let S be the first k indices of a STABLE ascending sort of the values
//                            (ties go to the lowest flat index); every element whose index is in S \ {0} becomes +0.0, every other
//                            element keeps its bits.  Flat index 0 (CLS -> CLS) is never zeroed but counts towards k.
//
// One 512-thread workgroup owns a matrix.  The values are non-negative, so they order as their uint32 bit patterns; the k-th
// smallest pattern v is found exactly by a most-significant-digit radix select, four passes of 8 bits:
//   1. every wave histograms the digit of the elements that match the prefix found so far into its OWN 256 bins in LDS (integer
//      adds: order-independent, so the kernel is deterministic).  Attention values crowd into a few exponent bins, so a wave first
//      folds the lanes that share the digit of its first active lane into one add (twice), then adds the rest one by one;
//   2. the bins of the waves are summed, and wave 0 scans the 256 totals for the bin that holds rank k - 1 and the rank inside it.
// After the four passes v, n_less = #{x < v} and n_eq = #{x == v} are known, and need = k - n_less of the elements equal to v go.
//   3. need == n_eq (no tie across the cut: the usual case): one pass zeroes every x <= v;
//      otherwise every wave takes a contiguous run of the matrix, counts its elements equal to v, and walks the run in index order
//      with a running count (ballot + popcount), zeroing x < v and the first `need` of x == v over the whole matrix.
// Every access is one dword at F + mat M + i with i < M: a matrix inside the slab is only 4-byte aligned (T is odd for every real
// ViT).  For negative or NaN input the selection runs on the bit patterns as they are: unspecified values, same accesses.
// No global atomics, no floating-point atomics, no workspace.
#include "cvcl_common.h"

namespace {

constexpr int DS_THREADS = 512;
constexpr int DS_WAVES = DS_THREADS / 64;
constexpr int DS_MAXT = 4096;                   // M = T T <= 2^24: every count fits 32 bits

// one element's digit into the wave's own bins; `active` false for the lanes past the end or off the prefix
__device__ __forceinline__ void ds_hist_add(unsigned* bins, bool active, unsigned d, int lane) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long act = __ballot(active);
        if (!act) return;                        // wave-uniform
        const int leader = __ffsll((long long)act) - 1;
        const unsigned dl = (unsigned)__shfl((int)d, leader, 64);
        const bool same = active && d == dl;
        const unsigned long long grp = __ballot(same);
        if (lane == leader) atomicAdd(&bins[dl], (unsigned)__popcll(grp));
        active = active && !same;
    }
    if (active) atomicAdd(&bins[d], 1u);         // ds_add_u32: the lanes that share a bin are serialised by the LDS
}

__global__ __launch_bounds__(DS_THREADS) void attention_discard_kernel(float* __restrict__ F, int M, unsigned k) {
    __shared__ unsigned hist[DS_WAVES][256];
    __shared__ unsigned total[256];
    __shared__ unsigned sel[3];                  // digit, elements below it, elements in it
    __shared__ unsigned wave_eq[DS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* m = reinterpret_cast<unsigned*>(F + (long)blockIdx.x * M);

    unsigned prefix = 0, rank = k - 1, n_less = 0, n_eq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        for (int b = lane; b < 256; b += 64) hist[wave][b] = 0;       // (own bins: ordered within the wave)
        for (int base = 0; base < M; base += 4 * DS_THREADS) {
            unsigned x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * DS_THREADS + tid;
                x[u] = i < M ? m[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * DS_THREADS + tid;
                ds_hist_add(hist[wave], i < M && (x[u] & himask) == prefix, (x[u] >> shift) & 255u, lane);
            }
        }
        __syncthreads();
        if (tid < 256) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < DS_WAVES; ++w) s += hist[w][tid];
            total[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {                         // bins 4 lane .. 4 lane + 3; rank < the sum of all bins, so exactly one lane holds it
            unsigned c[4], s = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) { c[u] = total[4 * lane + u]; s += c[u]; }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
                if (lane >= o) incl += t;
            }
            unsigned before = incl - s;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (before <= rank && rank < before + c[u]) {
                    sel[0] = 4 * lane + u;
                    sel[1] = before;
                    sel[2] = c[u];
                }
                before += c[u];
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        rank -= sel[1];
        n_less += sel[1];
        n_eq = sel[2];
        __syncthreads();                         // sel and the bins are free for the next pass
    }
    const unsigned v = prefix, need = k - n_less;                     // 1 <= need <= n_eq

    if (need == n_eq) {
        for (int i = tid; i < M; i += DS_THREADS)
            if (i != 0 && m[i] <= v) m[i] = 0u;
        return;
    }
    // a tie across the cut: wave w owns elements [w run, (w + 1) run)
    const int run = cvcl_div_up(M, DS_WAVES);
    const int lo = min(wave * run, M), hi = min(lo + run, M);
    unsigned cnt = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        cnt += (unsigned)__popcll(__ballot(i < hi && m[i] == v));
    }
    if (lane == 0) wave_eq[wave] = cnt;
    __syncthreads();
    unsigned seen = 0;                           // elements equal to v before this wave's run
    for (int w = 0; w < wave; ++w) seen += wave_eq[w];
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const unsigned x = i < hi ? m[i] : 0xffffffffu;
        const bool eq = i < hi && x == v;
        const unsigned long long b = __ballot(eq);
        const unsigned mine = seen + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
        if (i < hi && i != 0 && (x < v || (eq && mine < need))) m[i] = 0u;
        seen += (unsigned)__popcll(b);
    }
}

}  // namespace

extern "C" int cvcl_attention_discard(float* fused, int n_mats, int T, long k, void* stream) {
    CVCL_CHECK_ARG(fused, "cvcl_attention_discard: null fused");
    CVCL_CHECK_ARG(n_mats > 0, "cvcl_attention_discard: n_mats %d must be positive", n_mats);
    CVCL_CHECK_ARG(T >= 1 && T <= DS_MAXT, "cvcl_attention_discard: T %d outside 1 .. %d", T, DS_MAXT);
    const long M = (long)T * T;
    CVCL_CHECK_ARG(k >= 0 && k < M, "cvcl_attention_discard: k %ld outside 0 .. T*T - 1 = %ld", k, M - 1);
    if (k == 0) return CVCL_OK;                  // nothing to discard: no launch
    CvclProfScope prof(stream, CVCL_K_ATTENTION);
    hipLaunchKernelGGL(attention_discard_kernel, dim3((unsigned)n_mats), dim3(DS_THREADS), 0, (hipStream_t)stream, fused, (int)M,
                       (unsigned)k);
    CVCL_LAUNCH_CHECK();
    return CVCL_OK;
}
