// Thickness QC for gfx950: the local thickness of a squared-radius field (Hildebrand and Ruegsegger: per voxel the diameter of the
// largest ball that contains the voxel and stays inside the object), and the statistics of a float32 field under a byte mask.
//
//   oai_local_thickness   sq_out[p] = max over the centres q with d2(p, q) < rsq[q] of rsq[q], d2 the EDT's canonical expression in
//                         fp64 without contraction; thick[p] = 2 (float)sqrt(sq_out[p]).  To the bit of the brute force over all pairs
//                         (tests/local_thickness_ref.py)
//   oai_masked_stats      count, fp64 sums, min, max and np.percentile of the finite values that a byte mask admits
//
// The thickness is a scatter, so that the work is the sum of the centres' own windows and never the largest radius times the volume:
//   lt_init_kernel      the byte mask of the centres (rsq finite and > 0), their flags for the scan, the 64-bit key field zeroed
//   exclusive_scan_i32  (common.h) positions in the centre list; the list's length stays on the device
//   lt_compact_kernel   the list of centre voxels, in raster order
//   lt_scatter_kernel   one group of 16 lanes per centre, grid-stride over the list; a whole wave for a window above 1024 voxels.  The
//                       lanes walk the centre's clipped bounding window x-fastest; where d2 < rsq[q] and the byte says centre, the bit
//                       pattern of rsq[q] goes into the key of p by an integer atomicMax
//   lt_finish_kernel    key -> sq_out, thick; the counts
// Positive doubles order like their bit patterns, so the 64-bit integer max IS the fp64 max, and a max is commutative and associative:
// the atomics cost no reproducibility, every run gives the same bits whatever order the groups ran in.  This is the one place where
// the QC kernels use an atomic on a result, and why they may.  A relaxed load that already shows a key >= the candidate skips the
// atomic; a stale value there only costs an atomic that changes nothing.
#include "common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

#include "ordered_reduce.h"
#include "radix_select.h"

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kMaxAxis = 32767;
constexpr long long kMaxVoxels = 2147483647LL;     // the centre list and the scan are int32
constexpr int kG = 16;                             // lanes per centre (profiles/local_thickness.md: 16 against a whole wave) ...
constexpr long long kWide = 1024;                  // ... up to this many voxels in the window; above, the whole wave walks it
constexpr int kCounters = 8;                       // [1..3] of the stats; diagnostic builds: [4] covered centres met, [5] atomics issued
constexpr long long kScatterBlocks = 256LL * 8;
constexpr int kMS = 6;                             // doubles per block partial of masked_partials_kernel
constexpr int kRanks = kSelectRanks;
constexpr long long kStreamBlocks = 2048;          // 256 CUs x 8 blocks: grid-stride beyond that

__device__ __forceinline__ bool is_centre(double r) { return r > 0.0 && r < (double)INFINITY; }      // false for NaN

// ---- oai_local_thickness -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
lt_init_kernel(const double* __restrict__ rsq, long long n, unsigned char* __restrict__ centre, int* __restrict__ flag,
               unsigned long long* __restrict__ key, long long* __restrict__ counters) {
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i <= n; i += (long long)gridDim.x * kT) {
        if (i == n) { flag[n] = 0; break; }                        // the scan's last entry: the length of the list
        const bool c = is_centre(rsq[i]);
        centre[i] = c ? 1 : 0;
        flag[i] = c ? 1 : 0;
        key[i] = 0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x < kCounters) counters[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(kT)
lt_compact_kernel(const unsigned char* __restrict__ centre, const int* __restrict__ pos, long long n, int* __restrict__ list) {
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT)
        if (centre[i]) list[pos[i]] = (int)i;
}

// the largest k in [0, limit] with fl(((double)k * s)^2) < r2: the exact half-extent of the ball's bounding window on one axis.  The
// canonical d2 is >= each of its terms (adding a non-negative number never rounds below the other addend), so no voxel further out
// can pass.  floor(sqrt(r2) / s) + 1 is above the answer whatever the rounding of the square root and the quotient (their error is
// far below one voxel at k <= 32767); it is then walked down on the exact expression, two steps at the most unless the axis clipped it.
__device__ __forceinline__ int half_extent(double r2, double s, int limit) {
    const double guess = floor(sqrt(r2) / s) + 1.0;
    int k = guess < (double)limit ? (int)guess : limit;            // (also the huge radii: no conversion of an out-of-range double)
    for (; k > 0; --k) {
        const double t = (double)k * s;
        if (t * t < r2) break;
    }
    return k;
}

struct Window {                                                // a centre and the clipped bounding window of its ball
    double r2;
    int qx, qy, qz, x0, y0, z0, nx, ny, nz;
    __device__ __forceinline__ long long volume() const { return (long long)nx * ny * nz; }
};

__device__ __forceinline__ Window window_of(int q, const double* __restrict__ rsq, int D, int H, int W, double sx, double sy, double sz) {
    Window w;
    w.r2 = rsq[q];
    w.qx = q % W, w.qy = (q / W) % H, w.qz = q / (W * H);
    const int hx = half_extent(w.r2, sx, W - 1), hy = half_extent(w.r2, sy, H - 1), hz = half_extent(w.r2, sz, D - 1);
    w.x0 = max(w.qx - hx, 0), w.y0 = max(w.qy - hy, 0), w.z0 = max(w.qz - hz, 0);
    w.nx = min(w.qx + hx, W - 1) - w.x0 + 1, w.ny = min(w.qy + hy, H - 1) - w.y0 + 1, w.nz = min(w.qz + hz, D - 1) - w.z0 + 1;
    return w;
}

struct Tally {                                                 // diagnostic builds: covered centres met, atomics issued
#ifdef OAI_DIAG
    unsigned long long met = 0, issued = 0;
#endif
};

// raise the key of p to `bits` unless a relaxed load shows that it is there already (a stale value only costs an atomic)
__device__ __forceinline__ void raise_key(unsigned long long* key, long long p, unsigned long long bits, Tally& t) {
#ifdef OAI_DIAG
    t.met += 1;
#endif
    if (__hip_atomic_load(&key[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) {
#ifdef OAI_DIAG
        t.issued += 1;
#endif
        atomicMax(&key[p], bits);
    }
}

// lane `sub` of G takes the window's voxels sub, sub + G, ... in x-fastest order; G = (ez ny + ey) nx + ex is the step
template <int G>
__device__ __forceinline__ void walk_window(const Window& w, int sub, int H, int W, double sx, double sy, double sz,
                                            const unsigned char* __restrict__ centre, unsigned long long* __restrict__ key, Tally& t) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(w.r2);
    const int row = w.nx * w.ny;                                   // <= 32767^2 < 2^31
    const int ez = G / row, ey = (G % row) / w.nx, ex = G % w.nx;
    int dz = sub / row, dy = (sub % row) / w.nx, dx = sub % w.nx;
    while (dz < w.nz) {
        const int px = w.x0 + dx, py = w.y0 + dy, pz = w.z0 + dz;
        const double tx = (double)(px - w.qx) * sx, ty = (double)(py - w.qy) * sy, tz = (double)(pz - w.qz) * sz;
        const double d2 = (tx * tx + ty * ty) + tz * tz;
        if (d2 < w.r2) {
            const long long p = ((long long)pz * H + py) * W + px;
            if (centre[p]) raise_key(key, p, bits, t);
        }
        dx += ex;
        int carry = dx >= w.nx;
        dx -= carry ? w.nx : 0;
        dy += ey + carry;
        carry = dy >= w.ny;
        dy -= carry ? w.ny : 0;
        dz += ez + carry;
    }
}

// A wave takes 64 / G consecutive centres of the list at a time, grid-stride: group g of G lanes walks the window of centre g.  WIDE: a
// window above kWide voxels is left to the end of the round and then walked by the whole wave, one such centre after the other -- a
// large ball is a long serial walk for 16 lanes, and the time of the call is the time of its slowest group.  counters: [1] tests
// done, [2] capped centres, [3] the largest clipped window -- integers, exact in any order.
template <int G, bool WIDE>
__global__ void __launch_bounds__(kT)
lt_scatter_kernel(const double* __restrict__ rsq, const unsigned char* __restrict__ centre, const int* __restrict__ list,
                  const int* __restrict__ n_list, int D, int H, int W, double sx, double sy, double sz, long long cap,
                  unsigned long long* __restrict__ key, long long* __restrict__ counters) {
    const int count = *n_list;
    const int lane = threadIdx.x & 63, sub = lane % G;
    const long long groups = (long long)gridDim.x * (kT / G);
    long long work = 0, capped = 0, largest = 0;
    Tally tally;
    // `base` is the wave's first centre of the round: the loop is uniform over the wave, the ballot below sees every lane
    for (long long base = (long long)blockIdx.x * (kT / G) + (threadIdx.x >> 6) * (64 / G); base < count; base += groups) {
        const long long c = base + lane / G;
        int q = 0;
        bool wide = false;
        if (c < count) {
            q = list[c];
            const Window w = window_of(q, rsq, D, H, W, sx, sy, sz);
            const long long vol = w.volume();
            if (sub == 0) largest = max(largest, vol);
            if (vol > cap) {                                       // the guard: this centre covers itself and nothing else
                if (sub == 0) {
                    capped += 1;
                    work += 1;
                    raise_key(key, q, (unsigned long long)__double_as_longlong(w.r2), tally);
                }
            } else {
                if (sub == 0) work += vol;
                wide = WIDE && vol > kWide;
                if (!wide) walk_window<G>(w, sub, H, W, sx, sy, sz, centre, key, tally);
            }
        }
        if (WIDE) {
            unsigned long long todo = __ballot(wide && sub == 0);
            while (todo) {                                         // uniform: every lane holds the same mask
                const int leader = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const Window w = window_of(__shfl(q, leader, 64), rsq, D, H, W, sx, sy, sz);
                walk_window<64>(w, lane, H, W, sx, sy, sz, centre, key, tally);
            }
        }
    }
#ifdef OAI_DIAG
    if (tally.met) atomicAdd((unsigned long long*)&counters[4], tally.met);
    if (tally.issued) atomicAdd((unsigned long long*)&counters[5], tally.issued);
#endif
    if (sub == 0) {
        if (work) atomicAdd((unsigned long long*)&counters[1], (unsigned long long)work);
        if (capped) atomicAdd((unsigned long long*)&counters[2], (unsigned long long)capped);
        if (largest) atomicMax((unsigned long long*)&counters[3], (unsigned long long)largest);
    }
}

__global__ void __launch_bounds__(kT)
lt_finish_kernel(const unsigned long long* __restrict__ key, long long n, const int* __restrict__ n_list, const long long* __restrict__ counters,
                 double* __restrict__ sq_out, float* __restrict__ thick, long long* __restrict__ stats) {
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const double sq = __longlong_as_double((long long)key[i]);                 // 0 where p is not a centre: nothing was scattered there
        if (sq_out) sq_out[i] = sq;
        thick[i] = 2.0f * (float)sqrt(sq);
    }
    if (stats && blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = threadIdx.x == 0 ? (long long)*n_list : counters[threadIdx.x];
}

bool axes_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= kMaxAxis && H <= kMaxAxis && W <= kMaxAxis && (long long)D * H * W <= kMaxVoxels;
}

struct LtWs {
    unsigned long long* key;
    long long* counters;
    int *pos, *list, *scratch;
    unsigned char* centre;
    size_t bytes;
    LtWs(void* workspace, long long n) {
        Ws ws(workspace);
        key = ws.take<unsigned long long>((size_t)n);
        counters = ws.take<long long>(kCounters);
        pos = ws.take<int>((size_t)n + 1);
        list = ws.take<int>((size_t)n);
        scratch = ws.take<int>(scan_scratch_bytes(n + 1) / 4);
        centre = ws.take<unsigned char>((size_t)n);
        bytes = ws.off;
    }
};

// ---- oai_masked_stats ----------------------------------------------------------------------------------------------------------------
struct MaskedAcc {
    double v[kMS];                             // n, sum v, sum v^2, min, max, non-finite
    __device__ __forceinline__ void clear() { v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = INFINITY; v[4] = -INFINITY; v[5] = 0.0; }
    __device__ __forceinline__ void merge(const double* o) {       // this (the earlier elements) on the left of every operation
        v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = v[2] + o[2]; v[3] = fmin(v[3], o[3]); v[4] = fmax(v[4], o[4]); v[5] = v[5] + o[5];
    }
};

__device__ __forceinline__ bool admitted(const unsigned char* mask, long long i) { return !mask || mask[i] != 0; }

__global__ void __launch_bounds__(kT)
masked_partials_kernel(const float* __restrict__ values, const unsigned char* __restrict__ mask, long long n, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kMS];
    MaskedAcc acc;
    acc.clear();
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        if (!admitted(mask, i)) continue;
        const float f = values[i];
        if (!finite_f32(f)) { acc.v[5] = acc.v[5] + 1.0; continue; }
        const double d = (double)f;
        acc.v[0] = acc.v[0] + 1.0; acc.v[1] = acc.v[1] + d; acc.v[2] = acc.v[2] + d * d;
        acc.v[3] = fmin(acc.v[3], d); acc.v[4] = fmax(acc.v[4], d);
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kMS; ++i) partials[(long long)blockIdx.x * kMS + i] = acc.v[i];
}

struct MaskedSelect {                // lives in the caller's workspace
    SelectState sel;
    float gamma[kRanks / 2];         // numpy's interpolation weight of each percentile: known on the device only, like the count
};

// one block: the slots in the order of csrc/ordered_reduce.h; thread 0 writes out[0..4], out[7] and the ranks.  A rank not asked for is a
// copy of rank 0 (csrc/radix_select.h), as in surface_finish_kernel of csrc/edt.hip.
__global__ void __launch_bounds__(kT)
masked_finish_kernel(const double* __restrict__ partials, long long nb, float p0, float p1, int n_percentiles, MaskedSelect* st,
                     double* __restrict__ out) {
    __shared__ double lds[kT / 64][kMS];
    MaskedAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    select_clear_hist(&st->sel);
    if (threadIdx.x == 0) {
        const bool empty = acc.v[0] == 0.0;
        out[0] = acc.v[0];
        for (int i = 1; i < 5; ++i) out[i] = empty ? (double)NAN : acc.v[i];
        out[5] = out[6] = (double)NAN;                             // nothing counted, or a percentile not asked for
        out[7] = acc.v[5];
        const unsigned long long total = (unsigned long long)acc.v[0];
        unsigned long long first = 0;                              // rank 0
        for (int p = 0; p < kRanks / 2; ++p) {
            unsigned long long k0 = first, k1 = first;
            float g = 0.0f;
            if (!empty && p < n_percentiles) numpy_virtual_index(total, p == 0 ? p0 : p1, k0, k1, g);
            if (p == 0) first = k0;
            st->sel.prefix[2 * p] = st->sel.prefix[2 * p + 1] = 0;
            st->sel.rank[2 * p] = k0;
            st->sel.rank[2 * p + 1] = k1;
            st->gamma[p] = g;
        }
    }
}

__global__ void __launch_bounds__(kT)
masked_hist_kernel(const float* __restrict__ values, const unsigned char* __restrict__ mask, long long n, int pass, MaskedSelect* st) {
    select_hist_pass<kT>(&st->sel, pass, [&](auto add) {
        for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
            if (!admitted(mask, i)) continue;
            const float f = values[i];
            if (finite_f32(f)) add(f);
        }
    });
}

__global__ void __launch_bounds__(kT) masked_scan_kernel(int pass, MaskedSelect* st) { select_scan_step(&st->sel, pass); }

// nothing counted keeps its NaN
__global__ void masked_percentiles_kernel(const MaskedSelect* st, int n_percentiles, double* __restrict__ out) {
    const int p = threadIdx.x;
    if (p < n_percentiles && out[0] != 0.0) out[5 + p] = (double)numpy_lerp(st->sel.value[2 * p], st->sel.value[2 * p + 1], st->gamma[p]);
}

struct MaskedWs {
    double* partials;
    MaskedSelect* select;
    long long blocks;
    size_t bytes;
    MaskedWs(void* workspace, long long n) {
        Ws ws(workspace);
        blocks = n > 0 ? (long long)grid_stride_blocks(n, kT * 4, kStreamBlocks) : 0;
        partials = ws.take<double>((size_t)blocks * kMS);
        select = ws.take<MaskedSelect>(1);
        bytes = ws.off;
    }
};

}  // namespace

extern "C" {

size_t oai_local_thickness_workspace_bytes(int D, int H, int W) {
    if (!axes_ok(D, H, W)) return 0;
    return LtWs(nullptr, (long long)D * H * W).bytes;
}

int oai_local_thickness(const double* rsq_dev, int D, int H, int W, const double spacing_xyz[3], long long max_window_voxels,
                        double* sq_out_dev, float* thick_dev, void* workspace_dev, size_t workspace_bytes, long long* stats_dev, void* stream) {
    OAI_CHECK_ARG(axes_ok(D, H, W), "oai_local_thickness: every axis must be in [1, %d] and D*H*W <= 2^31 - 1 (got %d x %d x %d)", kMaxAxis, D, H, W);
    OAI_CHECK_ARG(rsq_dev && thick_dev && workspace_dev && spacing_xyz, "oai_local_thickness: null pointer");
    for (int c = 0; c < 3; ++c)
        OAI_CHECK_ARG(std::isfinite(spacing_xyz[c]) && spacing_xyz[c] > 0.0, "oai_local_thickness: spacing[%d] = %g must be finite and > 0", c,
                      spacing_xyz[c]);
    OAI_CHECK_ARG(max_window_voxels > 0, "oai_local_thickness: max_window_voxels must be > 0, got %lld", max_window_voxels);
    OAI_CHECK_WORKSPACE("oai_local_thickness", workspace_bytes, oai_local_thickness_workspace_bytes(D, H, W));
    const long long n = (long long)D * H * W;
    const LtWs ws(workspace_dev, n);
    const hipStream_t st = (hipStream_t)stream;
    lt_init_kernel<<<grid_stride_blocks(n + 1, kT), kT, 0, st>>>(rsq_dev, n, ws.centre, ws.pos, ws.key, ws.counters);
    OAI_CHECK_LAUNCH();
    if (int rc = exclusive_scan_i32(ws.pos, ws.pos, n + 1, ws.scratch, st)) return rc;
    lt_compact_kernel<<<grid_stride_blocks(n, kT), kT, 0, st>>>(ws.centre, ws.pos, n, ws.list);
    OAI_CHECK_LAUNCH();
    // the list's length is on the device only: the grid is sized by the volume, one group per voxel at the most
    const double sx = spacing_xyz[0], sy = spacing_xyz[1], sz = spacing_xyz[2];
    const int variant = diag_env("OAI_LT_GROUP", 0);               // diagnostic builds: 16 or 64 lanes per centre throughout (the variants that lost)
    const unsigned blocks16 = grid_stride_blocks(n, kT / kG, kScatterBlocks);
    if (variant == 64)
        lt_scatter_kernel<64, false><<<grid_stride_blocks(n, kT / 64, kScatterBlocks), kT, 0, st>>>(rsq_dev, ws.centre, ws.list, ws.pos + n, D, H, W, sx, sy,
                                                                                                  sz, max_window_voxels, ws.key, ws.counters);
    else if (variant == 16)
        lt_scatter_kernel<kG, false><<<blocks16, kT, 0, st>>>(rsq_dev, ws.centre, ws.list, ws.pos + n, D, H, W, sx, sy, sz, max_window_voxels, ws.key,
                                                              ws.counters);
    else
        lt_scatter_kernel<kG, true><<<blocks16, kT, 0, st>>>(rsq_dev, ws.centre, ws.list, ws.pos + n, D, H, W, sx, sy, sz, max_window_voxels, ws.key,
                                                             ws.counters);
    OAI_CHECK_LAUNCH();
    lt_finish_kernel<<<grid_stride_blocks(n, kT), kT, 0, st>>>(ws.key, n, ws.pos + n, ws.counters, sq_out_dev, thick_dev, stats_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_masked_stats_workspace_bytes(long long n) {
    if (n < 0) return 0;
    return MaskedWs(nullptr, n).bytes;
}

int oai_masked_stats(const float* values_dev, const unsigned char* mask_dev, long long n, const float* percentiles, int n_percentiles,
                     void* workspace_dev, size_t workspace_bytes, double* out_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_masked_stats: negative element count (%lld)", n);
    OAI_CHECK_ARG(out_dev && workspace_dev && (n == 0 || values_dev), "oai_masked_stats: null pointer");
    OAI_CHECK_ARG(n_percentiles >= 0 && n_percentiles <= kRanks / 2, "oai_masked_stats: 0 to %d percentiles, got %d", kRanks / 2, n_percentiles);
    OAI_CHECK_ARG(n_percentiles == 0 || percentiles, "oai_masked_stats: null pointer");
    for (int p = 0; p < n_percentiles; ++p)
        OAI_CHECK_ARG(percentiles[p] >= 0.0f && percentiles[p] <= 100.0f, "oai_masked_stats: percentile %g is outside [0, 100]", (double)percentiles[p]);
    OAI_CHECK_WORKSPACE("oai_masked_stats", workspace_bytes, oai_masked_stats_workspace_bytes(n));
    const MaskedWs ws(workspace_dev, n);
    const hipStream_t st = (hipStream_t)stream;
    if (ws.blocks) {
        masked_partials_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(values_dev, mask_dev, n, ws.partials);
        OAI_CHECK_LAUNCH();
    }
    masked_finish_kernel<<<1, kT, 0, st>>>(ws.partials, ws.blocks, n_percentiles > 0 ? percentiles[0] : 0.0f, n_percentiles > 1 ? percentiles[1] : 0.0f,
                                           n_percentiles, ws.select, out_dev);
    OAI_CHECK_LAUNCH();
    if (n_percentiles && ws.blocks) {
        for (int pass = 0; pass < 4; ++pass) {
            masked_hist_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(values_dev, mask_dev, n, pass, ws.select);
            OAI_CHECK_LAUNCH();
            masked_scan_kernel<<<1, kT, 0, st>>>(pass, ws.select);
            OAI_CHECK_LAUNCH();
        }
        masked_percentiles_kernel<<<1, 64, 0, st>>>(ws.select, n_percentiles, out_dev);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

}  // extern "C"
