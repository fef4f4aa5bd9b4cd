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

namespace {

using namespace oai;

constexpr int kT = 256;                        // threads per block: 64 x-adjacent lines, 4 positions along the line at a time
constexpr int kLines = 64;
constexpr int kMaxAxis = 32767;                // an offset fits 15 bits; 0xffff is free for "no feature"
constexpr unsigned kNoneX = 0xffffu;
constexpr unsigned kNoneXY = 0xffffffffu;
constexpr size_t kSlabBytes = 64 * 1024;       // a staged slab above this is read from global memory instead
constexpr int kSP = 6;                         // doubles per block partial of surface_partials_kernel: n_A, n_B, sums, maxima
constexpr int kRanks = 4;                      // two percentiles, two order statistics each
constexpr long long kStreamBlocks = 2048;      // 256 CUs x 8 blocks: grid-stride beyond that

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool in_set(float v, float thr) { return finite_f32(v) && v > thr; }

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

// one block: the feature count of the volume from the per-row counts (integers: exact in any order)
__global__ void __launch_bounds__(kT) edt_count_kernel(const unsigned* __restrict__ row_count, long long rows, long long* __restrict__ n_features) {
    __shared__ unsigned long long lds[kT / 64];
    unsigned long long acc = 0;
    for (long long i = threadIdx.x; i < rows; i += kT) acc += row_count[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kT / 64; ++w) acc += lds[w];
        *n_features = (long long)acc;
    }
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

// the block's kT accumulators into one, in a fixed order: shuffle tree inside each wave, then the waves in order.  Valid in thread 0.
__device__ __forceinline__ void block_reduce(SurfAcc& a, double (*lds)[kSP]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        double o[kSP];
#pragma unroll
        for (int i = 0; i < kSP; ++i) o[i] = __shfl_down(a.v[i], off, 64);
        a.merge(o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < kSP; ++i) lds[wave][i] = a.v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kT / 64; ++w) a.merge(lds[w]);
}

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
    block_reduce(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kSP; ++i) partials[(long long)blockIdx.x * kSP + i] = acc.v[i];
}

struct SelectState {                 // lives in the caller's workspace (the layout of csrc/normalize.hip's, plus the ranks' origin)
    unsigned prefix[kRanks];         // key bits fixed so far (high bits)
    unsigned long long rank[kRanks]; // remaining rank inside the current prefix bucket
    unsigned hist[kRanks][256];
    float value[kRanks];             // result: the order statistics
    float gamma[kRanks / 2];
};

__device__ __forceinline__ unsigned key_of(float f) {      // monotone float -> uint map (csrc/normalize.hip)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// np.percentile(a, q) on a float32 array of n elements: numpy_virtual_index of csrc/normalize.hip with the same float32 operations, on
// the device because n is known there only
__device__ void virtual_index(unsigned long long n, float pct, unsigned long long& k0, unsigned long long& k1, float& gamma) {
    const float q = pct / 100.0f;
    const float vi = (float)(n - 1) * q;
    float fl = floorf(vi);
    if (fl < 0.0f) fl = 0.0f;
    unsigned long long k = (unsigned long long)fl;
    gamma = vi - fl;
    if (k >= n - 1) { k = n - 1; gamma = 0.0f; }
    k0 = k;
    k1 = k + 1 < n ? k + 1 : n - 1;
}

// one block: thread t adds up its run of consecutive slots in index order, then the fixed tree; thread 0 writes out[0..5] and the ranks
__global__ void __launch_bounds__(kT)
surface_finish_kernel(const double* __restrict__ partials, long long nb, float p0, float p1, int n_percentiles, SelectState* st,
                      double* __restrict__ out) {
    __shared__ double lds[kT / 64][kSP];
    const long long per = (nb + kT - 1) / kT;
    const long long i0 = min(per * (long long)threadIdx.x, nb), i1 = min(i0 + per, nb);
    SurfAcc acc;
    acc.clear();
    for (long long i = i0; i < i1; ++i) acc.merge(partials + i * kSP);
    block_reduce(acc, lds);
    for (int i = threadIdx.x; i < kRanks * 256; i += kT) st->hist[i / 256][i % 256] = 0;
    if (threadIdx.x == 0) {
        const bool empty = acc.v[0] == 0.0 || acc.v[1] == 0.0;
        out[0] = acc.v[0];
        out[1] = acc.v[1];
        for (int i = 2; i < kSP; ++i) out[i] = empty ? (double)NAN : acc.v[i];
        out[6] = out[7] = (double)NAN;                             // an empty surface or a percentile not asked for
        const unsigned long long total = (unsigned long long)(acc.v[0] + acc.v[1]);
        for (int p = 0; p < kRanks / 2; ++p) {
            unsigned long long k0 = 0, k1 = 0;
            float g = 0.0f;
            if (!empty && p < n_percentiles) virtual_index(total, p == 0 ? p0 : p1, k0, k1, g);
            st->prefix[2 * p] = st->prefix[2 * p + 1] = 0;
            st->rank[2 * p] = k0;
            st->rank[2 * p + 1] = k1;
            st->gamma[p] = g;
        }
    }
}

// pass p (0 = most significant byte): histogram of byte p among the pooled distances whose higher bytes equal prefix[r]
__global__ void __launch_bounds__(kT)
surface_hist_kernel(const unsigned char* __restrict__ sa, const float* __restrict__ db, const unsigned char* __restrict__ sb,
                    const float* __restrict__ da, long long n, int pass, int n_ranks, SelectState* st) {
    __shared__ unsigned h[kRanks][256];
    for (int i = threadIdx.x; i < kRanks * 256; i += kT) h[i / 256][i % 256] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    unsigned pre[kRanks];
#pragma unroll
    for (int r = 0; r < kRanks; ++r) pre[r] = st->prefix[r];
    auto add = [&](float v) {
        const unsigned k = key_of(v), hi = k & mask, d = (k >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < kRanks; ++r)
            if (r < n_ranks && hi == pre[r]) atomicAdd(&h[r][d], 1u);
    };
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        if (sa[i]) add(db[i]);
        if (sb[i]) add(da[i]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRanks * 256; i += kT) {
        const unsigned v = h[i / 256][i % 256];
        if (v) atomicAdd(&st->hist[i / 256][i % 256], v);
    }
}

// one block: per rank, find the bin holding the rank, extend the prefix, clear the histograms for the next pass
__global__ void __launch_bounds__(kT) surface_scan_kernel(int pass, SelectState* st) {
    if (threadIdx.x < kRanks) {
        const int r = threadIdx.x;
        unsigned long long rem = st->rank[r];
        int d = 0;
        for (; d < 255; ++d) {
            const unsigned c = st->hist[r][d];
            if (rem < c) break;
            rem -= c;
        }
        const int shift = 24 - 8 * pass;
        st->rank[r] = rem;
        st->prefix[r] |= (unsigned)d << shift;
        if (pass == 3) st->value[r] = float_of(st->prefix[r]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRanks * 256; i += kT) st->hist[i / 256][i % 256] = 0;
}

// numpy's _lerp in the array dtype (float32), as window_params_kernel of csrc/normalize.hip; an empty surface keeps its NaN
__global__ void surface_percentiles_kernel(const SelectState* st, int n_percentiles, double* __restrict__ out) {
    const int p = threadIdx.x;
    if (p < n_percentiles && out[0] != 0.0 && out[1] != 0.0) {
        const float a = st->value[2 * p], b = st->value[2 * p + 1], t = st->gamma[p];
        const float diff = __fsub_rn(b, a);
        out[6 + p] = (double)(t < 0.5f ? __fadd_rn(a, __fmul_rn(diff, t)) : __fsub_rn(b, __fmul_rn(diff, __fsub_rn(1.0f, t))));
    }
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
    SelectState* select;
    long long blocks;
    size_t bytes;
    SurfWs(void* workspace, long long n) {
        Ws ws(workspace);
        blocks = n > 0 ? (long long)grid_stride_blocks(n, kT * 4, kStreamBlocks) : 0;
        partials = ws.take<double>((size_t)blocks * kSP);
        select = ws.take<SelectState>(1);
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
            surface_hist_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(surf_a_dev, dist_to_b_dev, surf_b_dev, dist_to_a_dev, n, pass, 2 * n_percentiles,
                                                                    ws.select);
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
