// Image-similarity QC for gfx950: what the registration was trained on (local normalised cross-correlation) and what the atlas was built
// under (normalised mutual information), of two float32 images on one grid.
//
//   oai_image_moments        counts and the six fp64 sums behind Pearson's r and the mean squared error
//   oai_joint_histogram      the bins x bins table of pairs, integer counts
//   oai_histogram_entropies  N and the three entropies of that table, on the device (the record stays one small download)
//   oai_lncc                 the fp64 map cc = cov / sqrt((var_a + eps)(var_b + eps)) of the five Gaussian-filtered moments, and its statistics
//
// fp64 with contraction off, written so that a numpy restatement performs the same operations in the same order
// (tests/similarity_ref.py).  Every floating sum goes through csrc/ordered_reduce.h: per-thread terms in a fixed order, one slot per
// block in the workspace, a one-block finish kernel -- no float atomics, a block count that depends on the shape only.  The histogram
// adds integers, which is exact in any order: LDS atomics per block, one 64-bit global atomic per non-zero cell when the block retires.
//
// oai_lncc is three passes, x then y then z, one thread per voxel with x on the lane (every load of a pass is a coalesced row piece):
//   lncc_x_kernel    reads a and b, forms a, b, aa, bb, ab in fp64 and filters them along x                -> plane set 0 (5 fp64 volumes)
//   lncc_y_kernel    filters plane set 0 along y                                                          -> plane set 1
//   lncc_z_kernel    filters plane set 1 along z, forms cc, writes the map if asked, reduces
// The taps of a row piece overlap in L1 / L2, so each pass moves its 40 B per voxel in and out of HBM once.  The x and y passes are not
// fused through LDS: at radius 32 a tile's x-filtered halo rows (5 fp64 channels) do not fit, and a second code path for small radii
// would have to be pinned to the same bits for a step that runs once per knee (profiles/image_similarity.md).
#include "common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

#include "ordered_reduce.h"

namespace {

using namespace oai;

constexpr int kT = 256;                       // threads per block
constexpr long long kStreamBlocks = 2048;     // oai_image_moments: 256 CUs x 8 blocks, grid-stride beyond that
constexpr long long kHistBlocks = 512;        // oai_joint_histogram: 2 blocks per CU, so that few tables are merged at the end
constexpr int kMaxBins = 128, kLdsBins = 64;  // a 64 x 64 uint32 table is 16 KB of LDS; above that, global atomics
constexpr int kMaxRadius = 32;
constexpr int kMP = 8;                        // doubles per partial of image_moments_kernel
constexpr int kLP = 6;                        // ... of lncc_z_kernel
constexpr int kCh = 5;                        // a, b, aa, bb, ab

// ---- oai_image_moments ---------------------------------------------------------------------------------------------------------------
struct MomAcc {
    double v[kMP];                            // counted, non-finite, sum a, sum b, sum aa, sum bb, sum ab, sum (a - b)^2
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < kMP; ++i) v[i] = 0.0;
    }
    __device__ __forceinline__ void merge(const double* o) {
#pragma unroll
        for (int i = 0; i < kMP; ++i) v[i] = v[i] + o[i];
    }
};

__global__ void __launch_bounds__(kT)
image_moments_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, const unsigned char* __restrict__ mask,
                     double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kMP];
    MomAcc acc;
    acc.clear();
    const long long stride = (long long)gridDim.x * kT;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        const float fa = a[i], fb = b[i];
        if (finite_f32(fa) && finite_f32(fb)) {
            const double da = (double)fa, db = (double)fb, d = da - db;
            acc.v[0] = acc.v[0] + 1.0;
            acc.v[2] = acc.v[2] + da;
            acc.v[3] = acc.v[3] + db;
            acc.v[4] = acc.v[4] + da * da;
            acc.v[5] = acc.v[5] + db * db;
            acc.v[6] = acc.v[6] + da * db;
            acc.v[7] = acc.v[7] + d * d;
        } else {
            acc.v[1] = acc.v[1] + 1.0;
        }
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kMP; ++i) partials[(long long)blockIdx.x * kMP + i] = acc.v[i];
}

__global__ void __launch_bounds__(kT)
image_moments_finish_kernel(const double* __restrict__ partials, long long nb, double* __restrict__ stats) {
    __shared__ double lds[kT / 64][kMP];
    MomAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kMP; ++i) stats[i] = acc.v[i];
}

long long moment_blocks(long long n) {
    const long long blocks = (n + 4 * kT - 1) / (4 * kT);
    return blocks > kStreamBlocks ? kStreamBlocks : blocks;
}

// ---- oai_joint_histogram -------------------------------------------------------------------------------------------------------------
struct HistArgs {
    float lo_a, hi_a, scale_a, lo_b, hi_b, scale_b;
    int bins;
};

// min((int)((clamp(x, lo, hi) - lo) * scale), bins - 1), every operation in float32
__device__ __forceinline__ int bin_of(float x, float lo, float hi, float scale, int bins) {
    const float c = fminf(fmaxf(x, lo), hi);
    const int k = (int)((c - lo) * scale);
    return min(k, bins - 1);
}

// LDS: the block's own table.  Folding runs of equal cells per thread (most pairs of a knee volume are background and land in cell
// (0,0)) was built and measured: within 5 % either way at 80x192x192, so it is not here (profiles/image_similarity.md).
template <bool LDS>
__global__ void __launch_bounds__(kT)
joint_histogram_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, HistArgs h, const unsigned char* __restrict__ mask,
                       unsigned long long* __restrict__ hist) {
    __shared__ unsigned int table[LDS ? kLdsBins * kLdsBins + 1 : 1];
    const int cells = h.bins * h.bins;
    if (LDS) {
        for (int c = threadIdx.x; c <= cells; c += kT) table[c] = 0u;
        __syncthreads();
    }
    auto add = [&](int cell, unsigned int count) {
        if (LDS)
            atomicAdd(&table[cell], count);
        else
            atomicAdd(&hist[cell], (unsigned long long)count);
    };
    unsigned int skipped = 0;
    const long long stride = (long long)gridDim.x * kT;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        const float fa = a[i], fb = b[i];
        if (!(finite_f32(fa) && finite_f32(fb))) {
            ++skipped;
            continue;
        }
        const int cell = bin_of(fa, h.lo_a, h.hi_a, h.scale_a, h.bins) * h.bins + bin_of(fb, h.lo_b, h.hi_b, h.scale_b, h.bins);
        add(cell, 1u);
    }
    if (skipped) add(cells, skipped);
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c <= cells; c += kT) {
            const unsigned int v = table[c];
            if (v) atomicAdd(&hist[c], (unsigned long long)v);
        }
    }
}

// ---- oai_histogram_entropies ---------------------------------------------------------------------------------------------------------
struct EntAcc {
    double v[3];                              // sum p log p of the marginal of a, of b, of the joint table
    __device__ __forceinline__ void clear() { v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; }
    __device__ __forceinline__ void merge(const double* o) { v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = v[2] + o[2]; }
};

__device__ __forceinline__ double plogp(long long c, double total) {
    const double p = (double)c / total;
    return p * log(p);
}

// one block.  Terms in index order: thread t takes its run of consecutive cells, then the ordered tree.
__global__ void __launch_bounds__(kT)
histogram_entropies_kernel(const long long* __restrict__ hist, int bins, double* __restrict__ out) {
    __shared__ long long marg[2][kMaxBins];
    __shared__ double lds[kT / 64][3];
    const int t = threadIdx.x, cells = bins * bins;
    if (t < bins) {                                                // marginal of a: the rows
        long long s = 0;
        for (int k = 0; k < bins; ++k) s += hist[t * bins + k];
        marg[0][t] = s;
    } else if (t >= kMaxBins && t - kMaxBins < bins) {             // marginal of b: the columns
        long long s = 0;
        for (int k = 0; k < bins; ++k) s += hist[k * bins + (t - kMaxBins)];
        marg[1][t - kMaxBins] = s;
    }
    __syncthreads();
    long long count = 0;
    for (int k = 0; k < bins; ++k) count += marg[0][k];
    const double total = (double)count;
    EntAcc acc;
    acc.clear();
    if (count > 0) {
        if (t < bins) {                                            // ceil(bins / 256) = 1 cell per thread
            if (marg[0][t] > 0) acc.v[0] = acc.v[0] + plogp(marg[0][t], total);
            if (marg[1][t] > 0) acc.v[1] = acc.v[1] + plogp(marg[1][t], total);
        }
        const int per = (cells + kT - 1) / kT, c0 = min(per * t, cells), c1 = min(c0 + per, cells);
        for (int c = c0; c < c1; ++c) {
            const long long v = hist[c];
            if (v > 0) acc.v[2] = acc.v[2] + plogp(v, total);
        }
    }
    block_reduce<kT>(acc, lds);
    if (t == 0) {
        out[0] = total;
        for (int i = 0; i < 3; ++i) out[1 + i] = count > 0 ? 0.0 - acc.v[i] : NAN;
    }
}

// ---- oai_lncc ------------------------------------------------------------------------------------------------------------------------
struct Taps {
    double w[2 * kMaxRadius + 1];
};

// numpy's np.pad(mode="reflect"), scipy's mode="mirror": no repeated edge sample.  n > radius, so one reflection is enough.
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ void __launch_bounds__(kT)
lncc_x_kernel(const float* __restrict__ a, const float* __restrict__ b, long long total, int W, Taps taps, int radius, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const long long row = i - x;
    double acc[kCh] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j <= 2 * radius; ++j) {
        const long long o = row + reflect(x + j - radius, W);
        const double w = taps.w[j], va = (double)a[o], vb = (double)b[o];
        acc[0] = acc[0] + w * va;
        acc[1] = acc[1] + w * vb;
        acc[2] = acc[2] + w * (va * va);
        acc[3] = acc[3] + w * (vb * vb);
        acc[4] = acc[4] + w * (va * vb);
    }
#pragma unroll
    for (int c = 0; c < kCh; ++c) dst[c * total + i] = acc[c];
}

__global__ void __launch_bounds__(kT)
lncc_y_kernel(const double* __restrict__ src, long long total, int H, int W, Taps taps, int radius, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= total) return;
    const int y = (int)((i / W) % H);
    const long long base = i - (long long)y * W;                   // the same x and z at y = 0
    double acc[kCh] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j <= 2 * radius; ++j) {
        const long long o = base + (long long)reflect(y + j - radius, H) * W;
        const double w = taps.w[j];
#pragma unroll
        for (int c = 0; c < kCh; ++c) acc[c] = acc[c] + w * src[c * total + o];
    }
#pragma unroll
    for (int c = 0; c < kCh; ++c) dst[c * total + i] = acc[c];
}

struct LnccAcc {
    double v[kLP];                            // counted, non-finite, sum cc, sum cc^2, min, max
    __device__ __forceinline__ void clear() { v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = INFINITY; v[5] = -INFINITY; }
    __device__ __forceinline__ void merge(const double* o) {
        v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = v[2] + o[2]; v[3] = v[3] + o[3]; v[4] = fmin(v[4], o[4]); v[5] = fmax(v[5], o[5]);
    }
};

// one voxel per thread, block b = voxels [256 b, 256 b + 256) in index order: the slots depend on the shape only
__global__ void __launch_bounds__(kT)
lncc_z_kernel(const double* __restrict__ src, long long total, int D, long long plane, Taps taps, int radius, double eps,
              const unsigned char* __restrict__ mask, double* __restrict__ cc_out, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kLP];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    LnccAcc st;
    st.clear();
    if (i < total) {
        const int z = (int)(i / plane);
        const long long base = i - (long long)z * plane;
        double acc[kCh] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j <= 2 * radius; ++j) {
            const long long o = base + (long long)reflect(z + j - radius, D) * plane;
            const double w = taps.w[j];
#pragma unroll
            for (int c = 0; c < kCh; ++c) acc[c] = acc[c] + w * src[c * total + o];
        }
        const double cov = acc[4] - acc[0] * acc[1];
        const double va = acc[2] - acc[0] * acc[0];
        const double vb = acc[3] - acc[1] * acc[1];
        const double cc = cov / sqrt((va + eps) * (vb + eps));
        if (cc_out) cc_out[i] = cc;
        if (!mask || mask[i]) {
            if (isfinite(cc)) {
                st.v[0] = st.v[0] + 1.0;
                st.v[2] = st.v[2] + cc;
                st.v[3] = st.v[3] + cc * cc;
                st.v[4] = fmin(st.v[4], cc);
                st.v[5] = fmax(st.v[5], cc);
            } else {
                st.v[1] = st.v[1] + 1.0;
            }
        }
    }
    block_reduce<kT>(st, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < kLP; ++k) partials[(long long)blockIdx.x * kLP + k] = st.v[k];
}

__global__ void __launch_bounds__(kT)
lncc_finish_kernel(const double* __restrict__ partials, long long nb, double* __restrict__ stats) {
    __shared__ double lds[kT / 64][kLP];
    LnccAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) stats[k] = acc.v[k];
        stats[4] = acc.v[0] > 0.0 ? acc.v[4] : NAN;
        stats[5] = acc.v[0] > 0.0 ? acc.v[5] : NAN;
    }
}

struct LnccWs {
    double *set0, *set1, *partials;
    long long total, nb;
};

bool lncc_shape_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1; }

size_t lncc_carve(Ws& ws, int D, int H, int W, LnccWs& w) {
    w.total = (long long)D * H * W;
    w.nb = (w.total + kT - 1) / kT;
    w.set0 = ws.take<double>((size_t)w.total * kCh);
    w.set1 = ws.take<double>((size_t)w.total * kCh);
    w.partials = ws.take<double>((size_t)w.nb * kLP);
    return ws.off;
}

}  // namespace

extern "C" {

size_t oai_image_moments_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    oai::Ws ws(nullptr);
    ws.take<double>((size_t)moment_blocks(n) * kMP);
    return ws.off;
}

int oai_image_moments(const float* a_dev, const float* b_dev, long long n, const unsigned char* mask_dev, void* workspace_dev, size_t workspace_bytes,
                      double* stats_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_image_moments: negative element count (%lld)", n);
    OAI_CHECK_ARG(stats_dev && (n == 0 || (a_dev && b_dev && workspace_dev)), "oai_image_moments: null pointer");
    OAI_CHECK_WORKSPACE("oai_image_moments", workspace_bytes, oai_image_moments_workspace_bytes(n));
    const hipStream_t st = (hipStream_t)stream;
    const long long nb = moment_blocks(n);
    double* partials = (double*)workspace_dev;
    if (nb) {
        image_moments_kernel<<<(unsigned)nb, kT, 0, st>>>(a_dev, b_dev, n, mask_dev, partials);
        OAI_CHECK_LAUNCH();
    }
    image_moments_finish_kernel<<<1, kT, 0, st>>>(partials, nb, stats_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_joint_histogram(const float* a_dev, const float* b_dev, long long n, const float range_a[2], const float range_b[2], int bins,
                        const unsigned char* mask_dev, long long* hist_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0 && n <= (1LL << 40), "oai_joint_histogram: element count %lld outside [0, 2^40]", n);
    OAI_CHECK_ARG(bins >= 1 && bins <= kMaxBins, "oai_joint_histogram: bins must be in [1, %d] (got %d)", kMaxBins, bins);
    OAI_CHECK_ARG(range_a && range_b && hist_dev && (n == 0 || (a_dev && b_dev)), "oai_joint_histogram: null pointer");
    // (the width itself must be a finite float32 as well: the kernel subtracts lo in float32)
    OAI_CHECK_ARG(std::isfinite(range_a[0]) && std::isfinite(range_a[1]) && range_a[1] > range_a[0] && std::isfinite(range_a[1] - range_a[0]) &&
                      std::isfinite(range_b[0]) && std::isfinite(range_b[1]) && range_b[1] > range_b[0] && std::isfinite(range_b[1] - range_b[0]),
                  "oai_joint_histogram: a range needs finite bounds with hi > lo (got [%g, %g] and [%g, %g])", (double)range_a[0],
                  (double)range_a[1], (double)range_b[0], (double)range_b[1]);
    HistArgs h;
    h.lo_a = range_a[0]; h.hi_a = range_a[1]; h.scale_a = (float)(bins / ((double)range_a[1] - (double)range_a[0]));
    h.lo_b = range_b[0]; h.hi_b = range_b[1]; h.scale_b = (float)(bins / ((double)range_b[1] - (double)range_b[0]));
    h.bins = bins;
    OAI_CHECK_ARG(std::isfinite(h.scale_a) && std::isfinite(h.scale_b), "oai_joint_histogram: a range too narrow for float32 (hi > lo by a normal amount)");
    const hipStream_t st = (hipStream_t)stream;
    OAI_CHECK_HIP(hipMemsetAsync(hist_dev, 0, ((size_t)bins * bins + 1) * sizeof(long long), st));
    if (n == 0) return OAI_OK;
    const unsigned nb = grid_stride_blocks(n, kT, kHistBlocks);
    unsigned long long* hist = (unsigned long long*)hist_dev;
    if (bins <= kLdsBins)
        joint_histogram_kernel<true><<<nb, kT, 0, st>>>(a_dev, b_dev, n, h, mask_dev, hist);
    else
        joint_histogram_kernel<false><<<nb, kT, 0, st>>>(a_dev, b_dev, n, h, mask_dev, hist);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_histogram_entropies(const long long* hist_dev, int bins, double* out_dev, void* stream) {
    OAI_CHECK_ARG(bins >= 1 && bins <= kMaxBins, "oai_histogram_entropies: bins must be in [1, %d] (got %d)", kMaxBins, bins);
    OAI_CHECK_ARG(hist_dev && out_dev, "oai_histogram_entropies: null pointer");
    histogram_entropies_kernel<<<1, kT, 0, (hipStream_t)stream>>>(hist_dev, bins, out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_lncc_workspace_bytes(int D, int H, int W) {
    if (!lncc_shape_ok(D, H, W)) return 0;
    oai::Ws ws(nullptr);
    LnccWs w;
    return lncc_carve(ws, D, H, W, w);
}

int oai_lncc(const float* a_dev, const float* b_dev, int D, int H, int W, const double* taps_host, int radius, double eps,
             const unsigned char* mask_dev, double* cc_out_dev, void* workspace_dev, size_t workspace_bytes, double* stats_dev, void* stream) {
    OAI_CHECK_ARG(radius >= 0 && radius <= kMaxRadius, "oai_lncc: radius must be in [0, %d] (got %d)", kMaxRadius, radius);
    OAI_CHECK_ARG(lncc_shape_ok(D, H, W) && D > radius && H > radius && W > radius,
                  "oai_lncc: every axis must be longer than the radius %d, reflect padding is undefined otherwise (got %d x %d x %d)", radius, D, H, W);
    OAI_CHECK_ARG(a_dev && b_dev && taps_host && workspace_dev && stats_dev, "oai_lncc: null pointer");
    OAI_CHECK_ARG(std::isfinite(eps) && eps >= 0.0, "oai_lncc: eps must be finite and >= 0 (got %g)", eps);
    oai::Ws ws(workspace_dev);
    LnccWs w;
    const size_t need = lncc_carve(ws, D, H, W, w);
    OAI_CHECK_ARG(w.nb <= 0x7fffffffLL, "oai_lncc: %d x %d x %d is too large for one launch", D, H, W);
    OAI_CHECK_WORKSPACE("oai_lncc", workspace_bytes, need);
    Taps taps;
    for (int j = 0; j < 2 * kMaxRadius + 1; ++j) taps.w[j] = j <= 2 * radius ? taps_host[j] : 0.0;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)w.nb;
    lncc_x_kernel<<<nb, kT, 0, st>>>(a_dev, b_dev, w.total, W, taps, radius, w.set0);
    OAI_CHECK_LAUNCH();
    lncc_y_kernel<<<nb, kT, 0, st>>>(w.set0, w.total, H, W, taps, radius, w.set1);
    OAI_CHECK_LAUNCH();
    lncc_z_kernel<<<nb, kT, 0, st>>>(w.set1, w.total, D, (long long)H * W, taps, radius, eps, mask_dev, cc_out_dev, w.partials);
    OAI_CHECK_LAUNCH();
    lncc_finish_kernel<<<1, kT, 0, st>>>(w.partials, w.nb, stats_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
