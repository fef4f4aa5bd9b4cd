// Exact order statistics of float32 values on the device, and numpy's percentile arithmetic on them: the shared core of
// oai_image_normalize (csrc/normalize.hip: the intensity window) and oai_surface_distance (csrc/edt.hip: the pooled percentiles).
//
// A 4-pass 8-bit radix select over the order-preserving integer image of the floats, kSelectRanks ranks at once (two percentiles,
// the order statistics k and k + 1 of each).  Per pass: select_hist_pass in a grid-stride kernel (LDS-privatised histograms of the
// pass's byte among the values whose higher bytes equal a rank's prefix), then select_scan_step in a one-block kernel (per rank the bin
// holding it; the prefix grows by one byte; the histograms are cleared for the next pass).  The counts are integers, so every order
// statistic is exact.  Ranks whose prefixes are equal share one histogram row (k and k + 1 almost always do): an owner with fewer
// ranks to find initialises the others as copies of rank 0, which then cost no atomics.
// Each owner keeps a SelectState in its workspace beside its own extras, and feeds select_hist_pass its values.
#pragma once
#include <hip/hip_runtime.h>

namespace oai {

constexpr int kSelectRanks = 4;

struct SelectState {                        // lives in the caller's workspace
    unsigned prefix[kSelectRanks];          // key bits fixed so far (high bits)
    unsigned long long rank[kSelectRanks];  // remaining rank inside the current prefix bucket
    unsigned hist[kSelectRanks][256];
    float value[kSelectRanks];              // result: the order statistics
};

__device__ __forceinline__ unsigned key_of(float f) {      // monotone float -> uint map
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// np.percentile(a, q) on a float32 array of n elements, numpy >= 2 semantics: the quantile, the virtual index and gamma are float32
__host__ __device__ inline void numpy_virtual_index(unsigned long long n, float pct, unsigned long long& k0, unsigned long long& k1, float& gamma) {
#pragma clang fp contract(off)
    const float q = pct / 100.0f;                       // np.true_divide(q, a.dtype.type(100))
    const float vi = (float)(n - 1) * q;                // (n - 1) * quantiles
    float fl = floorf(vi);
    if (fl < 0.0f) fl = 0.0f;
    unsigned long long k = (unsigned long long)fl;
    gamma = vi - fl;
    if (k >= n - 1) { k = n - 1; gamma = 0.0f; }        // virtual_indexes >= n-1 -> the last element
    k0 = k;
    k1 = k + 1 < n ? k + 1 : n - 1;
}

// numpy's _lerp in the array dtype (float32): a + (b-a)*t for t < 0.5, else b - (b-a)*(1-t); no FMA contraction
__device__ __forceinline__ float numpy_lerp(float a, float b, float t) {
    const float diff = __fsub_rn(b, a);
    return t < 0.5f ? __fadd_rn(a, __fmul_rn(diff, t)) : __fsub_rn(b, __fmul_rn(diff, __fsub_rn(1.0f, t)));
}

__device__ __forceinline__ void select_clear_hist(SelectState* st) {      // by every thread of one block
    for (int i = threadIdx.x; i < kSelectRanks * 256; i += blockDim.x) st->hist[i / 256][i % 256] = 0;
}

// Pass p (0 = most significant byte), by every thread of a kT-thread block of a grid: the histogram of byte p among the values whose
// higher bytes equal prefix[r].  for_each(add) calls add(v) for each of this thread's values.
template <int kT, class ForEach>
__device__ __forceinline__ void select_hist_pass(SelectState* st, int pass, ForEach for_each) {
    __shared__ unsigned h[kSelectRanks][256];
    for (int i = threadIdx.x; i < kSelectRanks * 256; i += kT) h[i / 256][i % 256] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    unsigned pre[kSelectRanks];
#pragma unroll
    for (int r = 0; r < kSelectRanks; ++r) pre[r] = st->prefix[r];
    const bool same01 = pre[0] == pre[1], same23 = pre[2] == pre[3], same02 = pre[0] == pre[2];
    for_each([&](float v) {
        const unsigned k = key_of(v);
        const unsigned hi = k & mask, d = (k >> shift) & 255u;
        // ranks that share a prefix share a histogram row: count once, select_scan_step reads the shared row
        if (hi == pre[0]) atomicAdd(&h[0][d], 1u);
        if (!same01 && hi == pre[1]) atomicAdd(&h[1][d], 1u);
        if (!same02 && hi == pre[2]) atomicAdd(&h[2][d], 1u);
        if (!same23 && !(pre[3] == pre[0]) && hi == pre[3]) atomicAdd(&h[3][d], 1u);
    });
    __syncthreads();
    for (int i = threadIdx.x; i < kSelectRanks * 256; i += kT) {
        const unsigned v = h[i / 256][i % 256];
        if (v) atomicAdd(&st->hist[i / 256][i % 256], v);
    }
}

// By every thread of one block: per rank, find the bin holding the rank, extend the prefix, clear the histograms for the next pass
__device__ __forceinline__ void select_scan_step(SelectState* st, int pass) {
    unsigned pre[kSelectRanks];
#pragma unroll
    for (int r = 0; r < kSelectRanks; ++r) pre[r] = st->prefix[r];
    __syncthreads();                                      // every thread holds all the prefixes before one of them is extended
    if (threadIdx.x < kSelectRanks) {
        const int r = threadIdx.x;
        const unsigned mine = r == 0 ? pre[0] : r == 1 ? pre[1] : r == 2 ? pre[2] : pre[3];
        // the histogram row this rank's prefix was counted in (see select_hist_pass)
        int row = r;
        if (r == 1 && pre[1] == pre[0]) row = 0;
        if (r == 2 && pre[2] == pre[0]) row = 0;
        if (r == 3) row = pre[3] == pre[0] ? 0 : (pre[3] == pre[2] ? (pre[2] == pre[0] ? 0 : 2) : 3);
        unsigned long long rem = st->rank[r];
        int d = 0;
        for (; d < 255; ++d) {
            const unsigned c = st->hist[row][d];
            if (rem < c) break;
            rem -= c;
        }
        const int shift = 24 - 8 * pass;
        st->rank[r] = rem;
        st->prefix[r] = mine | ((unsigned)d << shift);
        if (pass == 3) st->value[r] = float_of(mine | (unsigned)d);
    }
    __syncthreads();
    select_clear_hist(st);
}

}  // namespace oai
