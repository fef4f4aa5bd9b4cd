// Surface-distance QC for gfx950: the exact Euclidean distance transform of a binary volume with anisotropic spacing, the surface of a
// thresholded map, and the surface-distance figures (ASSD, Hausdorff, pooled percentiles) of two surfaces.
//
//   oai_mask_surface      the set `finite and > threshold` (oai_mask_overlap's rule), its 6-neighbour surface, or its complement, as bytes
//   oai_edt               per voxel the minimum over all feature voxels q of  (tx*tx + ty*ty) + tz*tz,  t = (double)(p - q) * spacing,
//                         in fp64 without contraction: what scipy.ndimage.distance_transform_edt(sampling=) computes, to the bit of the
//                         brute-force minimum (tests/edt_ref.py)
//   oai_surface_distance  counts, fp64 sums, maxima and np.percentile of the pooled directed distances (MedPy's assd / hd / hd95)
//
// The transform is separable and every pass searches its line exhaustively up to an exact cut-off, so no parabola intersection is ever
// computed in floating point:
//   edt_x_kernel   one row per wave; "last feature seen" prefix and suffix scans in 64-voxel chunks; |dx| to the row's nearest feature
//                  as uint16 (0xffff: none in the row)
//   edt_y_kernel   a block stages the 64 x-adjacent columns of one z slice ([H][64] uint16) in LDS, global access coalesced along x;
//                  each thread scans outward from its own voxel, k = 0, 1, 2, ..., candidates at y - k and y + k, and keeps the
//                  integer pair (|dx|, |dy|) minimising tx*tx + ty*ty
//   edt_z_kernel   the same along z over the [D][64] uint32 pairs; writes the squared distance and the float32 distance
// IEEE rounding is monotone (a <= b  =>  fl(a + c) <= fl(b + c)), so the minimum of the canonical expression over a line's candidates is
// the canonical expression on the minimal partial sum, and a scan may stop at the first k with fl((k s)^2) >= best: no later candidate
// can be smaller.  Intermediate state is integer offsets (2 + 4 bytes per voxel of workspace), never a rounded distance.  A line too long
// for 64 KB of LDS (H > 512, D > 256) is read from global memory by the same code.
#include "common.h"

#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

#include "ordered_reduce.h"
#include "radix_select.h"

namespace {

using namespace oai;

constexpr int kT = 256;                        // threads per block: 64 x-adjacent lines, 4 positions along the line at a time
constexpr int kLines = 64;
constexpr int kMaxAxis = 32767;                // an offset fits 15 bits; 0xffff is free for "no feature"
constexpr unsigned kNoneX = 0xffffu;
constexpr unsigned kNoneXY = 0xffffffffu;
constexpr size_t kSlabBytes = 64 * 1024;       // a staged slab above this is read from global memory instead
constexpr int kSP = 6;                         // doubles per block partial of surface_partials_kernel: n_A, n_B, sums, maxima
constexpr int kRanks = kSelectRanks;           // two percentiles, two order statistics each
constexpr long long kStreamBlocks = 2048;      // 256 CUs x 8 blocks: grid-stride beyond that

// ---- oai_mask_surface ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
mask_surface_kernel(const float* __restrict__ map, int D, int H, int W, float thr, int mode, unsigned char* __restrict__ out) {
    const long long n = (long long)D * H * W, plane = (long long)H * W;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const bool s = in_set(map[i], thr);
        bool r = mode == 2 ? !s : s;
        if (mode == 1 && s) {
            const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / plane);
            bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && z > 0 && z < D - 1;
            if (inner)
                inner = in_set(map[i - 1], thr) && in_set(map[i + 1], thr) && in_set(map[i - W], thr) && in_set(map[i + W], thr) &&
                        in_set(map[i - plane], thr) && in_set(map[i + plane], thr);
            r = !inner;
        }
        out[i] = r ? 1 : 0;
    }
}

// ---- oai_edt -------------------------------------------------------------------------------------------------------------------------
// one row per wave.  dx is read back by the thread that wrote it.
__global__ void __launch_bounds__(kT)
edt_x_kernel(const unsigned char* __restrict__ feat, long long rows, int W, unsigned short* dx, unsigned* __restrict__ row_count) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                       // the whole wave leaves; the kernel has no block barrier
    const unsigned char* f = feat + row * W;
    unsigned short* d = dx + row * W;
    unsigned count = 0;
    int carry = -1;                                                // the last feature at or before x, left to right
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool is = x < W && f[x] != 0;
        count += is;
        int last = is ? x : -1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(last, off, 64);
            if (lane >= off) last = max(last, o);
        }
        last = max(last, carry);
        carry = __shfl(last, 63, 64);
        if (x < W) d[x] = (unsigned short)(last < 0 ? kNoneX : (unsigned)(x - last));
    }
    carry = INT_MAX;                                               // the first feature at or after x, right to left
    for (int x0 = (W - 1) / 64 * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        const bool is = x < W && f[x] != 0;
        int next = is ? x : INT_MAX;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(next, off, 64);
            if (lane + off < 64) next = min(next, o);
        }
        next = min(next, carry);
        carry = __shfl(next, 0, 64);
        if (x < W) {
            const unsigned left = d[x], right = next == INT_MAX ? kNoneX : (unsigned)(next - x);
            d[x] = (unsigned short)min(left, right);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) count += __shfl_down(count, off, 64);
    if (lane == 0) row_count[row] = count;
}

struct CountAcc {
    unsigned long long v[1];
    __device__ __forceinline__ void clear() { v[0] = 0; }
    __device__ __forceinline__ void merge(const unsigned long long* o) { v[0] += o[0]; }
};

// one block: the feature count of the volume from the per-row counts (integers: exact in any order)
__global__ void __launch_bounds__(kT) edt_count_kernel(const unsigned* __restrict__ row_count, long long rows, long long* __restrict__ n_features) {
    __shared__ unsigned long long lds[kT / 64][1];
    CountAcc acc;
    acc.clear();
    for (long long i = threadIdx.x; i < rows; i += kT) acc.v[0] += row_count[i];
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) *n_features = (long long)acc.v[0];
}

// The outward scan of one line of `len` entries from position `pos`: k = 0, 1, 2, ..., entries pos - k and pos + k.  at(j, k, t2) takes
// the candidate at entry j, t2 = fl((k step)^2) being its term of the canonical expression; open(t2) says whether t2 is still below
// the best sum so far.  The scan ends at the first k where it is not: by the monotonicity above no later candidate can win.
template <class At, class Open>
__device__ __forceinline__ void scan_line(int pos, int len, double step, At at, Open open) {
    for (int k = 0;; ++k) {
        const bool lo = pos - k >= 0, hi = pos + k < len;
        if (!lo && !hi) break;
        const double t = (double)k * step;
        const double t2 = t * t;
        if (!open(t2)) break;
        if (lo) at(pos - k, k, t2);
        if (hi && k) at(pos + k, k, t2);
    }
}

extern __shared__ __align__(16) unsigned char edt_slab[];

// block (bx, z): columns x = 64 bx + lane of slice z, all H entries
template <bool LDS>
__global__ void __launch_bounds__(kT)
edt_y_kernel(const unsigned short* __restrict__ dx, int H, int W, int nbx, double sx, double sy, unsigned* __restrict__ xy) {
    unsigned short* slab = reinterpret_cast<unsigned short*>(edt_slab);
    const int bx = (int)(blockIdx.x % (unsigned)nbx), z = (int)(blockIdx.x / (unsigned)nbx);
    const int lane = threadIdx.x & 63, x = bx * kLines + lane, phase = threadIdx.x >> 6;
    const long long base = (long long)z * H * W + x;
    if (LDS) {
        for (int y = phase; y < H; y += kT / 64) slab[y * kLines + lane] = x < W ? dx[base + (long long)y * W] : (unsigned short)kNoneX;
        __syncthreads();
    }
    if (x >= W) return;
    for (int y = phase; y < H; y += kT / 64) {
        double best = INFINITY;
        unsigned pair = kNoneXY;
        scan_line(y, H, sy,
                  [&](int j, int k, double ty2) {
                      const unsigned d = LDS ? slab[j * kLines + lane] : dx[base + (long long)j * W];
                      if (d != kNoneX) {
                          const double tx = (double)d * sx;
                          const double s = tx * tx + ty2;
                          if (s < best) { best = s; pair = d | ((unsigned)k << 16); }
                      }
                  },
                  [&](double ty2) { return ty2 < best; });
        xy[base + (long long)y * W] = pair;
    }
}

// block (bx, y): lines x = 64 bx + lane of row y, all D entries
template <bool LDS>
__global__ void __launch_bounds__(kT)
edt_z_kernel(const unsigned* __restrict__ xy, int D, int H, int W, int nbx, double sx, double sy, double sz, float scale, int accumulate,
             float* __restrict__ dist, double* __restrict__ sq_out) {
    unsigned* slab = reinterpret_cast<unsigned*>(edt_slab);
    const int bx = (int)(blockIdx.x % (unsigned)nbx), y = (int)(blockIdx.x / (unsigned)nbx);
    const int lane = threadIdx.x & 63, x = bx * kLines + lane, phase = threadIdx.x >> 6;
    const long long plane = (long long)H * W, base = (long long)y * W + x;
    if (LDS) {
        for (int z = phase; z < D; z += kT / 64) slab[z * kLines + lane] = x < W ? xy[base + z * plane] : kNoneXY;
        __syncthreads();
    }
    if (x >= W) return;
    for (int z = phase; z < D; z += kT / 64) {
        double best = INFINITY;
        scan_line(z, D, sz,
                  [&](int j, int, double tz2) {
                      const unsigned p = LDS ? slab[j * kLines + lane] : xy[base + j * plane];
                      if (p != kNoneXY) {
                          const double tx = (double)(p & 0xffffu) * sx, ty = (double)(p >> 16) * sy;
                          const double s = (tx * tx + ty * ty) + tz2;
                          if (s < best) best = s;
                      }
                  },
                  [&](double tz2) { return tz2 < best; });
        const long long o = base + z * plane;
        if (sq_out) sq_out[o] = best;
        const float d = scale * (float)sqrt(best);
        dist[o] = (accumulate ? dist[o] : 0.0f) + d;
    }
}

// ---- oai_surface_distance ------------------------------------------------------------------------------------------------------------
struct SurfAcc {
    double v[kSP];                             // n_A, n_B, sum d(A->B), sum d(B->A), max d(A->B), max d(B->A)
    __device__ __forceinline__ void clear() { v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = -INFINITY; v[5] = -INFINITY; }
    __device__ __forceinline__ void merge(const double* o) {       // this (the earlier voxels) on the left of every sum
        v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = v[2] + o[2]; v[3] = v[3] + o[3]; v[4] = fmax(v[4], o[4]); v[5] = fmax(v[5], o[5]);
    }
};

__global__ void __launch_bounds__(kT)
surface_partials_kernel(const unsigned char* __restrict__ sa, const float* __restrict__ db, const unsigned char* __restrict__ sb,
                        const float* __restrict__ da, long long n, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kSP];
    SurfAcc acc;
    acc.clear();
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        if (sa[i]) {
            const double d = (double)db[i];
            acc.v[0] = acc.v[0] + 1.0; acc.v[2] = acc.v[2] + d; acc.v[4] = fmax(acc.v[4], d);
        }
        if (sb[i]) {
            const double d = (double)da[i];
            acc.v[1] = acc.v[1] + 1.0; acc.v[3] = acc.v[3] + d; acc.v[5] = fmax(acc.v[5], d);
        }
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kSP; ++i) partials[(long long)blockIdx.x * kSP + i] = acc.v[i];
}

struct SurfSelect {                  // lives in the caller's workspace
    SelectState sel;
    float gamma[kRanks / 2];         // numpy's interpolation weight of each percentile: known on the device only, like the pooled count
};

// one block: the slots in the order of csrc/ordered_reduce.h; thread 0 writes out[0..5] and the ranks.  A rank not asked for is a copy of
// rank 0: it shares rank 0's histogram row in every pass, and its value is never read.
__global__ void __launch_bounds__(kT)
surface_finish_kernel(const double* __restrict__ partials, long long nb, float p0, float p1, int n_percentiles, SurfSelect* st,
                      double* __restrict__ out) {
    __shared__ double lds[kT / 64][kSP];
    SurfAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    select_clear_hist(&st->sel);
    if (threadIdx.x == 0) {
        const bool empty = acc.v[0] == 0.0 || acc.v[1] == 0.0;
        out[0] = acc.v[0];
        out[1] = acc.v[1];
        for (int i = 2; i < kSP; ++i) out[i] = empty ? (double)NAN : acc.v[i];
        out[6] = out[7] = (double)NAN;                             // an empty surface or a percentile not asked for
        const unsigned long long total = (unsigned long long)(acc.v[0] + acc.v[1]);
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

// one pass of the select over the pooled directed distances
__global__ void __launch_bounds__(kT)
surface_hist_kernel(const unsigned char* __restrict__ sa, const float* __restrict__ db, const unsigned char* __restrict__ sb,
                    const float* __restrict__ da, long long n, int pass, SurfSelect* st) {
    select_hist_pass<kT>(&st->sel, pass, [&](auto add) {
        for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
            if (sa[i]) add(db[i]);
            if (sb[i]) add(da[i]);
        }
    });
}

__global__ void __launch_bounds__(kT) surface_scan_kernel(int pass, SurfSelect* st) { select_scan_step(&st->sel, pass); }

// an empty surface keeps its NaN
__global__ void surface_percentiles_kernel(const SurfSelect* st, int n_percentiles, double* __restrict__ out) {
    const int p = threadIdx.x;
    if (p < n_percentiles && out[0] != 0.0 && out[1] != 0.0)
        out[6 + p] = (double)numpy_lerp(st->sel.value[2 * p], st->sel.value[2 * p + 1], st->gamma[p]);
}

bool axes_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= kMaxAxis && H <= kMaxAxis && W <= kMaxAxis; }

struct EdtWs {
    unsigned short* dx;
    unsigned* xy;
    unsigned* row_count;
    size_t bytes;
    EdtWs(void* workspace, int D, int H, int W) {
        Ws ws(workspace);
        const size_t n = (size_t)D * H * W;
        dx = ws.take<unsigned short>(n);
        xy = ws.take<unsigned>(n);
        row_count = ws.take<unsigned>((size_t)D * H);
        bytes = ws.off;
    }
};

struct SurfWs {
    double* partials;
    SurfSelect* select;
    long long blocks;
    size_t bytes;
    SurfWs(void* workspace, long long n) {
        Ws ws(workspace);
        blocks = n > 0 ? (long long)grid_stride_blocks(n, kT * 4, kStreamBlocks) : 0;
        partials = ws.take<double>((size_t)blocks * kSP);
        select = ws.take<SurfSelect>(1);
        bytes = ws.off;
    }
};

}  // namespace

extern "C" {

int oai_mask_surface(const float* map_dev, int D, int H, int W, float threshold, int mode, unsigned char* out_dev, void* stream) {
    OAI_CHECK_ARG(axes_ok(D, H, W), "oai_mask_surface: every axis must be in [1, %d] (got %d x %d x %d)", kMaxAxis, D, H, W);
    OAI_CHECK_ARG(map_dev && out_dev, "oai_mask_surface: null pointer");
    OAI_CHECK_ARG(mode >= 0 && mode <= 2, "oai_mask_surface: mode must be 0 (set), 1 (surface) or 2 (complement), got %d", mode);
    OAI_CHECK_ARG(!std::isnan(threshold), "oai_mask_surface: the threshold is NaN");
    const long long n = (long long)D * H * W;
    mask_surface_kernel<<<grid_stride_blocks(n, kT), kT, 0, (hipStream_t)stream>>>(map_dev, D, H, W, threshold, mode, out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_edt_workspace_bytes(int D, int H, int W) {
    if (!axes_ok(D, H, W)) return 0;
    return EdtWs(nullptr, D, H, W).bytes;
}

int oai_edt(const unsigned char* feature_dev, int D, int H, int W, const double spacing_xyz[3], float scale, int accumulate, float* dist_dev,
            double* sq_out_dev, void* workspace_dev, size_t workspace_bytes, long long* n_features_dev, void* stream) {
    OAI_CHECK_ARG(axes_ok(D, H, W), "oai_edt: every axis must be in [1, %d] (got %d x %d x %d)", kMaxAxis, D, H, W);
    OAI_CHECK_ARG(feature_dev && dist_dev && workspace_dev && spacing_xyz, "oai_edt: null pointer");
    for (int c = 0; c < 3; ++c)
        OAI_CHECK_ARG(std::isfinite(spacing_xyz[c]) && spacing_xyz[c] > 0.0, "oai_edt: spacing[%d] = %g must be finite and > 0", c, spacing_xyz[c]);
    OAI_CHECK_ARG(scale == 1.0f || scale == -1.0f, "oai_edt: scale must be 1 or -1, got %g", (double)scale);
    OAI_CHECK_WORKSPACE("oai_edt", workspace_bytes, oai_edt_workspace_bytes(D, H, W));
    const EdtWs ws(workspace_dev, D, H, W);
    const hipStream_t st = (hipStream_t)stream;
    const double sx = spacing_xyz[0], sy = spacing_xyz[1], sz = spacing_xyz[2];
    const long long rows = (long long)D * H;
    const int nbx = (int)cdiv(W, kLines);
    edt_x_kernel<<<cdiv(rows, kT / 64), kT, 0, st>>>(feature_dev, rows, W, ws.dx, ws.row_count);
    OAI_CHECK_LAUNCH();
    if (n_features_dev) {
        edt_count_kernel<<<1, kT, 0, st>>>(ws.row_count, rows, n_features_dev);
        OAI_CHECK_LAUNCH();
    }
    const size_t slab_y = (size_t)H * kLines * sizeof(unsigned short), slab_z = (size_t)D * kLines * sizeof(unsigned);
    if (slab_y <= kSlabBytes)
        edt_y_kernel<true><<<(unsigned)nbx * (unsigned)D, kT, slab_y, st>>>(ws.dx, H, W, nbx, sx, sy, ws.xy);
    else
        edt_y_kernel<false><<<(unsigned)nbx * (unsigned)D, kT, 0, st>>>(ws.dx, H, W, nbx, sx, sy, ws.xy);
    OAI_CHECK_LAUNCH();
    if (slab_z <= kSlabBytes)
        edt_z_kernel<true><<<(unsigned)nbx * (unsigned)H, kT, slab_z, st>>>(ws.xy, D, H, W, nbx, sx, sy, sz, scale, accumulate, dist_dev, sq_out_dev);
    else
        edt_z_kernel<false><<<(unsigned)nbx * (unsigned)H, kT, 0, st>>>(ws.xy, D, H, W, nbx, sx, sy, sz, scale, accumulate, dist_dev, sq_out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_surface_distance_workspace_bytes(long long n) {
    if (n < 0) return 0;
    return SurfWs(nullptr, n).bytes;
}

int oai_surface_distance(const unsigned char* surf_a_dev, const float* dist_to_b_dev, const unsigned char* surf_b_dev, const float* dist_to_a_dev,
                         long long n, const float* percentiles, int n_percentiles, void* workspace_dev, size_t workspace_bytes, double* out_dev,
                         void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_surface_distance: negative element count (%lld)", n);
    OAI_CHECK_ARG(out_dev && workspace_dev && (n == 0 || (surf_a_dev && dist_to_b_dev && surf_b_dev && dist_to_a_dev)),
                  "oai_surface_distance: null pointer");
    OAI_CHECK_ARG(n_percentiles >= 0 && n_percentiles <= kRanks / 2, "oai_surface_distance: 0 to %d percentiles, got %d", kRanks / 2, n_percentiles);
    OAI_CHECK_ARG(n_percentiles == 0 || percentiles, "oai_surface_distance: null pointer");
    for (int p = 0; p < n_percentiles; ++p)
        OAI_CHECK_ARG(percentiles[p] >= 0.0f && percentiles[p] <= 100.0f, "oai_surface_distance: percentile %g is outside [0, 100]", (double)percentiles[p]);
    OAI_CHECK_WORKSPACE("oai_surface_distance", workspace_bytes, oai_surface_distance_workspace_bytes(n));
    const SurfWs ws(workspace_dev, n);
    const hipStream_t st = (hipStream_t)stream;
    if (ws.blocks) {
        surface_partials_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(surf_a_dev, dist_to_b_dev, surf_b_dev, dist_to_a_dev, n, ws.partials);
        OAI_CHECK_LAUNCH();
    }
    surface_finish_kernel<<<1, kT, 0, st>>>(ws.partials, ws.blocks, n_percentiles > 0 ? percentiles[0] : 0.0f, n_percentiles > 1 ? percentiles[1] : 0.0f,
                                            n_percentiles, ws.select, out_dev);
    OAI_CHECK_LAUNCH();
    if (n_percentiles && ws.blocks) {
        for (int pass = 0; pass < 4; ++pass) {
            surface_hist_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(surf_a_dev, dist_to_b_dev, surf_b_dev, dist_to_a_dev, n, pass, ws.select);
            OAI_CHECK_LAUNCH();
            surface_scan_kernel<<<1, kT, 0, st>>>(pass, ws.select);
            OAI_CHECK_LAUNCH();
        }
        surface_percentiles_kernel<<<1, 64, 0, st>>>(ws.select, n_percentiles, out_dev);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

}  // extern "C"
