// Atlas thickness map for gfx950: the step after get_thickness_mesh (SURVEY row L1').
//
// Replaces, on the device, the two calls FullDemo.ipynb makes after the per-point thickness (oai_analysis/mesh_processing.py:400-534):
//   map_attributes(source, target)        vtkPointInterpolator + SetNullPointsStrategyToClosestPoint   -> oai_map_attributes(_grid)
//   project_thickness(mapped, mesh_type)  FC: least-squares circle (scipy leastsq) + angle             -> oai_fit_circle + oai_project_circle
//                                         TC: KernelPCA(linear) per plateau, rotations, flip, offset   -> oai_project_plateaus
//
// map_attributes restates VTK 9's defaults (vtk is not installed, so this half is unpinned): vtkLinearKernel (every point inside the
// footprint weighs the same), the RADIUS footprint with Radius 1.0, NormalizeWeights on -> the plain mean over source points with
// |p - q|^2 <= r^2; no point inside -> the closest source point's value (ties: the smallest index).  Sums are fp64 in a fixed order
// (grid: cell by cell, each cell's list in ascending point index; brute force: ascending index), stored as float32.
// oai_point_footprint(_grid) is the same walk with no point array: it returns what decides mean versus fallback -- the count inside the
// radius, the closest squared distance and its source index -- so that a caller can tell "no cartilage here" from a thickness.
//
// project_thickness: a linear-kernel PCA equals the PCA of the 3x3 scatter matrix, so each plateau needs O(n) work (three
// deterministic fp64 reductions) and a 3x3 eigen-decomposition on the host instead of sklearn's n x n kernel matrix.  The sign of each
// component follows sklearn's svd_flip(u): the point with the largest |score| gets a positive score (first index on a tie).
//
// Reductions are block partials (a fixed number of blocks, a fixed tree in LDS) plus one final block: no float atomics, the same bits
// on every run.  Everything here is latency- or gather-bound VALU work; nothing is GEMM-shaped.
#include "common.h"
#include "uniform_grid.h"

#include <cmath>
#include <utility>

namespace {

constexpr int kT = 256;              // threads per block
constexpr int kRedBlocks = 256;      // blocks of every reduction (the partials' layout depends on nothing but n)
constexpr int kMaxComp = 4;          // point-array components interpolated per launch
constexpr int kSrcTile = 512;        // brute force: source points staged in LDS per step
constexpr float kSplitZ = 50.0f;     // project_thickness TC: plateaus split at z < 50 (raw coordinate units, :489-493)

// fp64 squared distance of two float32 points, without contraction: the bits numpy gets from dx*dx + dy*dy + dz*dz
__device__ __forceinline__ double dist2(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
    return dx * dx + dy * dy + dz * dz;
}

// ---------------------------------------------------------------------------------------------------------------------
// point binning: cells of size h >= radius, count -> scan -> scatter, then each cell's list ordered by point index
// ---------------------------------------------------------------------------------------------------------------------
using oai::UniformGrid;

__global__ void __launch_bounds__(kT) bin_count_kernel(const float* __restrict__ src, long long n, UniformGrid g, int* __restrict__ cell_of,
                                                       int* __restrict__ count) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int c = oai::grid_index(g, oai::grid_cell(g, 0, src[3 * i]), oai::grid_cell(g, 1, src[3 * i + 1]), oai::grid_cell(g, 2, src[3 * i + 2]));
    cell_of[i] = c;
    atomicAdd(&count[c], 1);
}

__global__ void __launch_bounds__(kT) bin_scatter_kernel(const int* __restrict__ cell_of, long long n, const int* __restrict__ start,
                                                         int* __restrict__ cursor, int* __restrict__ unordered) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of[i];
    unordered[start[c] + atomicAdd(&cursor[c], 1)] = (int)i;
}

// a point's rank in its cell = the number of cell members with a smaller index (the indices are distinct): O(cell size) per point
__global__ void __launch_bounds__(kT) bin_order_kernel(const int* __restrict__ unordered, long long n, const int* __restrict__ cell_of,
                                                       const int* __restrict__ start, int* __restrict__ list) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const int idx = unordered[p], c = cell_of[idx], s = start[c], e = start[c + 1];
    int rank = 0;
    for (int k = s; k < e; ++k) rank += unordered[k] < idx;
    list[s + rank] = idx;
}

// ---------------------------------------------------------------------------------------------------------------------
// interpolation: mean over the radius footprint, else the closest source point
// ---------------------------------------------------------------------------------------------------------------------
struct Interp {
    const float* vals;        // [nc][n_src] (already offset to the first component of this launch)
    long long n_src;
    int nc;                   // <= kMaxComp
    float* out;               // [nc][n_tgt]
    long long n_tgt;
    int* count;               // oai_point_footprint (nc = 0, no values): the footprint itself, [n_tgt] each; null in map_attributes
    double* nearest_d2;
    int* nearest_j;
};

struct Acc {
    double sum[kMaxComp];
    int cnt;
    double best;              // closest squared distance so far, its source index
    int best_j;
};

__device__ __forceinline__ void acc_point(Acc& a, const Interp& ip, double d2, double r2, int j) {
    if (d2 <= r2) {
        ++a.cnt;
#pragma unroll
        for (int m = 0; m < kMaxComp; ++m)
            if (m < ip.nc) a.sum[m] += (double)ip.vals[m * ip.n_src + j];
    }
    if (d2 < a.best || (d2 == a.best && j < a.best_j)) { a.best = d2; a.best_j = j; }
}

__device__ __forceinline__ void acc_store(const Acc& a, const Interp& ip, long long i) {
#pragma unroll
    for (int m = 0; m < kMaxComp; ++m) {
        if (m >= ip.nc) break;
        float v;
        if (a.cnt > 0) v = (float)(a.sum[m] / (double)a.cnt);
        else v = a.best_j >= 0 ? ip.vals[m * ip.n_src + a.best_j] : __int_as_float(0x7fc00000);     // no finite source point: NaN
        ip.out[m * ip.n_tgt + i] = v;
    }
    if (ip.count) { ip.count[i] = a.cnt; ip.nearest_d2[i] = a.best; ip.nearest_j[i] = a.best_j; }
}

__global__ void __launch_bounds__(kT) interp_grid_kernel(const float* __restrict__ src, const float* __restrict__ tgt, UniformGrid g, double r2,
                                                         const int* __restrict__ start, const int* __restrict__ list, Interp ip) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= ip.n_tgt) return;
    const float q[3] = {tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2]};
    // a target outside the grid starts from the clamped cell: the cells hold every source point, and the distance from q to a point of
    // the grid box is at least the distance from q's projection onto the box, so the ring bound below still holds
    const int cx = oai::grid_cell(g, 0, q[0]), cy = oai::grid_cell(g, 1, q[1]), cz = oai::grid_cell(g, 2, q[2]);
    Acc a;
#pragma unroll
    for (int m = 0; m < kMaxComp; ++m) a.sum[m] = 0.0;
    a.cnt = 0; a.best = INFINITY; a.best_j = -1;
    auto visit = [&](int x, int y, int z) {
        const int cell = oai::grid_index(g, x, y, z);
        for (int k = start[cell]; k < start[cell + 1]; ++k) {
            const int j = list[k];
            acc_point(a, ip, dist2(src + 3 * (long long)j, q), r2, j);
        }
    };
    // the footprint: h >= radius, so every source point within the radius lies in the 27 cells around q's (clamping keeps that).
    // One box walk, not shell 0 then shell 1: the sums are accumulated in visit order
    oai::grid_walk_box(max(cx - 1, 0), max(cy - 1, 0), max(cz - 1, 0), min(cx + 1, g.n[0] - 1), min(cy + 1, g.n[1] - 1), min(cz + 1, g.n[2] - 1), visit);
    if (a.cnt == 0) {
        // closest point: shells of Chebyshev radius r >= 2 around q's cell.  A point not visited after shell r-1 is at least (r-1) h
        // away; stop once the best is strictly closer than that (strict: an unvisited point at exactly that distance could win the
        // tie by a smaller index)
        // for q outside the grid box, |q - s|^2 >= |q - Pq|^2 + |Pq - s|^2 for every s in the box (Pq: q's projection onto it)
        double out2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double lo = g.lo[k], hi = g.lo[k] + g.n[k] * g.h, v = (double)q[k];
            const double e = v < lo ? lo - v : (v > hi ? v - hi : 0.0);
            out2 += e * e;
        }
        const int rmax = oai::grid_rmax(g, cx, cy, cz);
        for (int r = 2; r <= rmax; ++r) {
            const double covered = (double)(r - 1) * g.h;
            if (a.best < out2 + covered * covered) break;
            oai::grid_walk_shell(g, cx, cy, cz, r, visit);
        }
    }
    acc_store(a, ip, i);
}

// the same result without a grid (broad_phase=False): every source point, ascending index -- the library's cross-check
__global__ void __launch_bounds__(kT) interp_brute_kernel(const float* __restrict__ src, const float* __restrict__ tgt, double r2, Interp ip) {
    __shared__ float tile[kSrcTile * 3];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool live = i < ip.n_tgt;
    const float q[3] = {live ? tgt[3 * i] : 0.f, live ? tgt[3 * i + 1] : 0.f, live ? tgt[3 * i + 2] : 0.f};
    Acc a;
#pragma unroll
    for (int m = 0; m < kMaxComp; ++m) a.sum[m] = 0.0;
    a.cnt = 0; a.best = INFINITY; a.best_j = -1;
    for (long long j0 = 0; j0 < ip.n_src; j0 += kSrcTile) {
        const int cnt = (int)(ip.n_src - j0 < kSrcTile ? ip.n_src - j0 : kSrcTile);
        __syncthreads();
        for (int k = threadIdx.x; k < 3 * cnt; k += kT) tile[k] = src[3 * j0 + k];
        __syncthreads();
        if (live)
            for (int k = 0; k < cnt; ++k) acc_point(a, ip, dist2(tile + 3 * k, q), r2, (int)(j0 + k));
    }
    if (live) acc_store(a, ip, i);
}

// ---------------------------------------------------------------------------------------------------------------------
// deterministic fp64 reductions: kRedBlocks partials (grid-stride in a fixed pattern, fixed LDS tree), then one block
// ---------------------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void block_sum_store(const double (&v)[K], double* __restrict__ dst) {
    __shared__ double sh[K][kT];
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        __syncthreads();
    }
    if ((int)threadIdx.x < K) dst[threadIdx.x] = sh[threadIdx.x][0];
}

template <int K>
__global__ void __launch_bounds__(kT) final_sum_kernel(const double* __restrict__ partials, double* __restrict__ out) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (int)threadIdx.x < kRedBlocks ? partials[threadIdx.x * K + k] : 0.0;
    block_sum_store<K>(v, out);
}

// mask: 0 every point, 1 z < kSplitZ (left plateau), 2 z >= kSplitZ (right plateau); a NaN z is in neither half, as in the reference
__device__ __forceinline__ bool selected(float z, int mask) { return mask == 0 || (mask == 1 ? z < kSplitZ : z >= kSplitZ); }

// {count, sum d (3), sum d d^T (xx xy xz yy yz zz)} with d = p - ref over the masked points
__global__ void __launch_bounds__(kT) moments_kernel(const float* __restrict__ pts, long long n, int mask, double r0, double r1, double r2,
                                                     double* __restrict__ partials) {
    double v[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)kRedBlocks * kT) {
        if (!selected(pts[3 * i + 2], mask)) continue;
        const double dx = (double)pts[3 * i] - r0, dy = (double)pts[3 * i + 1] - r1, dz = (double)pts[3 * i + 2] - r2;
        v[0] += 1.0; v[1] += dx; v[2] += dy; v[3] += dz;
        v[4] += dx * dx; v[5] += dx * dy; v[6] += dx * dz; v[7] += dy * dy; v[8] += dy * dz; v[9] += dz * dz;
    }
    block_sum_store<10>(v, partials + blockIdx.x * 10);
}

// the nine sums of one circle-fit step at centre c: R_i = |c - p_i|, d_i = (c - p_i) / R_i over (x, y) = (p[col_x], p[col_y]):
// {sum R, sum R^2, sum d (2), sum d d^T (xx xy yy), sum d R (2)}
__global__ void __launch_bounds__(kT) circle_sums_kernel(const float* __restrict__ pts, long long n, int col_x, int col_y, double c0, double c1,
                                                         double* __restrict__ partials) {
    double v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)kRedBlocks * kT) {
        const double dx = c0 - (double)pts[3 * i + col_x], dy = c1 - (double)pts[3 * i + col_y];
        const double R = sqrt(dx * dx + dy * dy);
        const double ux = dx / R, uy = dy / R;
        v[0] += R; v[1] += R * R; v[2] += ux; v[3] += uy;
        v[4] += ux * ux; v[5] += ux * uy; v[6] += uy * uy; v[7] += ux * R; v[8] += uy * R;
    }
    block_sum_store<9>(v, partials + blockIdx.x * 9);
}

// svd_flip(u): per component, the masked point with the largest |score| (first index on a tie) and its signed score
struct Ext {
    double a, v;
    long long i;
};

__device__ __forceinline__ bool ext_better(const Ext& x, const Ext& y) { return x.a > y.a || (x.a == y.a && x.i < y.i); }

struct Axes {
    double mean[3];
    double u[2][3];
};

__device__ __forceinline__ double score(const float* __restrict__ p, const Axes& ax, int k) {
    return ax.u[k][0] * ((double)p[0] - ax.mean[0]) + ax.u[k][1] * ((double)p[1] - ax.mean[1]) + ax.u[k][2] * ((double)p[2] - ax.mean[2]);
}

__device__ __forceinline__ void block_ext_store(Ext (&e)[2], Ext* __restrict__ dst) {
    __shared__ Ext sh[2][kT];
    sh[0][threadIdx.x] = e[0];
    sh[1][threadIdx.x] = e[1];
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 2; ++k)
                if (ext_better(sh[k][threadIdx.x + s], sh[k][threadIdx.x])) sh[k][threadIdx.x] = sh[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 2) dst[threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void __launch_bounds__(kT) score_extreme_kernel(const float* __restrict__ pts, long long n, int mask, Axes ax, Ext* __restrict__ partials) {
    Ext e[2] = {{-1.0, 0.0, (long long)1 << 62}, {-1.0, 0.0, (long long)1 << 62}};
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)kRedBlocks * kT) {
        if (!selected(pts[3 * i + 2], mask)) continue;
        for (int k = 0; k < 2; ++k) {
            const double s = score(pts + 3 * i, ax, k);
            const Ext c = {fabs(s), s, i};
            if (ext_better(c, e[k])) e[k] = c;
        }
    }
    block_ext_store(e, partials + blockIdx.x * 2);
}

__global__ void __launch_bounds__(kT) final_ext_kernel(const Ext* __restrict__ partials, Ext* __restrict__ out) {
    Ext e[2];
    for (int k = 0; k < 2; ++k) e[k] = (int)threadIdx.x < kRedBlocks ? partials[threadIdx.x * 2 + k] : Ext{-1.0, 0.0, (long long)1 << 62};
    block_ext_store(e, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// per-point projections (fp64)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) circle_project_kernel(const float* __restrict__ pts, long long n, int col_x, int col_y, double c0, double c1,
                                                            double* __restrict__ angle, double* __restrict__ z) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    angle[i] = atan2((double)pts[3 * i + col_y] - c1, (double)pts[3 * i + col_x] - c0);
    z[i] = (double)pts[3 * i + 2];
}

__global__ void __launch_bounds__(kT) half_flags_kernel(const float* __restrict__ pts, long long n, int* __restrict__ right, int* __restrict__ left) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    const float z = i < n ? pts[3 * i + 2] : NAN;       // element n: 0 in both, so that the scans end on the totals
    right[i] = z >= kSplitZ;
    left[i] = z < kSplitZ;
}

// a plateau's map: scores on its two (sign-fixed) axes, then (s0, s1) @ [[c, -s], [s, c]], x scaled by fx, oy added to y
struct HalfMap {
    Axes ax;
    double c, s, fx, oy;
};

__global__ void __launch_bounds__(kT) plateau_project_kernel(const float* __restrict__ pts, const float* __restrict__ vals, long long n,
                                                             HalfMap right, HalfMap left, const int* __restrict__ off_right,
                                                             const int* __restrict__ off_left, long long n_right, double* __restrict__ ox,
                                                             double* __restrict__ oy, double* __restrict__ ov) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float z = pts[3 * i + 2];
    long long slot;
    const HalfMap* m;
    if (z >= kSplitZ) { slot = off_right[i]; m = &right; }                   // output: the right plateau first, then the left one
    else if (z < kSplitZ) { slot = n_right + off_left[i]; m = &left; }
    else return;
    const double s0 = score(pts + 3 * i, m->ax, 0), s1 = score(pts + 3 * i, m->ax, 1);
    ox[slot] = m->fx * (s0 * m->c + s1 * m->s);
    oy[slot] = (-s0 * m->s + s1 * m->c) + m->oy;
    ov[slot] = (double)vals[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Workspaces: one struct of typed pointers per entry-point family, filled by one carve() that returns the bytes walked (oai::Ws,
// common.h): over a null base that is the *_workspace_bytes answer, over the caller's buffer the carving.
struct PointGridWs { int *cell_of, *count, *start, *unordered, *list, *scratch; };
size_t carve(PointGridWs& w, const void* base, long long ncells, long long n_src) {
    oai::Ws ws(base);
    w.cell_of = ws.take<int>(n_src);
    w.count = ws.take<int>(ncells + 1);
    w.start = ws.take<int>(ncells + 1);
    w.unordered = ws.take<int>(n_src);
    w.list = ws.take<int>(n_src);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(ncells + 1) / 4);
    return ws.off;
}

struct MapWs { double *partials, *sums; Ext *ext_partials, *ext; int *right, *left, *off_right, *off_left, *scratch; };
size_t carve(MapWs& w, const void* base, long long n) {
    oai::Ws ws(base);
    w.partials = ws.take<double>(kRedBlocks * 16);
    w.sums = ws.take<double>(16);
    w.ext_partials = ws.take<Ext>(kRedBlocks * 2);
    w.ext = ws.take<Ext>(2);
    w.right = ws.take<int>(n + 1);
    w.left = ws.take<int>(n + 1);
    w.off_right = ws.take<int>(n + 1);
    w.off_left = ws.take<int>(n + 1);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(n + 1) / 4);
    return ws.off;
}

int launch_interp(bool grid, const float* src, long long n_src, const float* vals, int n_comp, const float* tgt, long long n_tgt, double radius,
                  const UniformGrid& g, const int* start, const int* list, float* out, hipStream_t st) {
    const double r2 = radius * radius;
    for (int c0 = 0; c0 < n_comp; c0 += kMaxComp) {
        Interp ip{vals + (long long)c0 * n_src, n_src, n_comp - c0 < kMaxComp ? n_comp - c0 : kMaxComp, out + (long long)c0 * n_tgt, n_tgt,
                  nullptr, nullptr, nullptr};
        if (grid) interp_grid_kernel<<<oai::cdiv(n_tgt, kT), kT, 0, st>>>(src, tgt, g, r2, start, list, ip);
        else interp_brute_kernel<<<oai::cdiv(n_tgt, kT), kT, 0, st>>>(src, tgt, r2, ip);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

// the source points into their cells: count -> scan -> scatter -> each cell's list in ascending point index
int bin_points(const float* src, long long n_src, const UniformGrid& g, const PointGridWs& w, hipStream_t st) {
    const long long ncells = (long long)g.n[0] * g.n[1] * g.n[2];
    if (int rc = oai::bucket_clear(w.count, ncells, st)) return rc;
    bin_count_kernel<<<oai::cdiv(n_src, kT), kT, 0, st>>>(src, n_src, g, w.cell_of, w.count);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::bucket_starts(w.count, w.start, ncells, w.scratch, st)) return rc;
    bin_scatter_kernel<<<oai::cdiv(n_src, kT), kT, 0, st>>>(w.cell_of, n_src, w.start, w.count, w.unordered);
    OAI_CHECK_LAUNCH();
    bin_order_kernel<<<oai::cdiv(n_src, kT), kT, 0, st>>>(w.unordered, n_src, w.cell_of, w.start, w.list);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// oai_point_footprint: the interpolation kernels with no point array (nc = 0: nothing summed, nothing stored but the footprint)
int launch_footprint(bool grid, const float* src, long long n_src, const float* tgt, long long n_tgt, double radius, const UniformGrid& g, const int* start,
                     const int* list, int* count, double* nearest_d2, int* nearest_j, hipStream_t st) {
    const Interp ip{nullptr, n_src, 0, nullptr, n_tgt, count, nearest_d2, nearest_j};
    if (grid) interp_grid_kernel<<<oai::cdiv(n_tgt, kT), kT, 0, st>>>(src, tgt, g, radius * radius, start, list, ip);
    else interp_brute_kernel<<<oai::cdiv(n_tgt, kT), kT, 0, st>>>(src, tgt, radius * radius, ip);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// the reductions' results come back to the host: these calls synchronise the stream
int read_sums(double* dev, double* host, int k, hipStream_t st) {
    OAI_CHECK_HIP(hipMemcpyAsync(host, dev, k * sizeof(double), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    return OAI_OK;
}

int moments(const float* pts, long long n, int mask, const double ref[3], const MapWs& w, double out[10], hipStream_t st) {
    moments_kernel<<<kRedBlocks, kT, 0, st>>>(pts, n, mask, ref[0], ref[1], ref[2], w.partials);
    OAI_CHECK_LAUNCH();
    final_sum_kernel<10><<<1, kT, 0, st>>>(w.partials, w.sums);
    OAI_CHECK_LAUNCH();
    return read_sums(w.sums, out, 10, st);
}

int circle_sums(const float* pts, long long n, int cx, int cy, const double c[2], const MapWs& w, double out[9], hipStream_t st) {
    circle_sums_kernel<<<kRedBlocks, kT, 0, st>>>(pts, n, cx, cy, c[0], c[1], w.partials);
    OAI_CHECK_LAUNCH();
    final_sum_kernel<9><<<1, kT, 0, st>>>(w.partials, w.sums);
    OAI_CHECK_LAUNCH();
    return read_sums(w.sums, out, 9, st);
}

// eigen-decomposition of a symmetric 3x3 matrix (cyclic Jacobi); columns of V are the eigenvectors, w descending
void eig_sym3(const double S[3][3], double w[3], double V[3][3]) {
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[i][j] = S[i][j]; V[i][j] = i == j; }
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off == 0.0 || off <= 1e-36 * diag) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {          // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {          // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {          // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (A[order[j]][order[j]] > A[order[i]][order[i]]) std::swap(order[i], order[j]);
    double W[3][3];
    for (int k = 0; k < 3; ++k) {
        w[k] = A[order[k]][order[k]];
        for (int i = 0; i < 3; ++i) W[i][k] = V[i][order[k]];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = W[i][j];
}

// one plateau: mean, centred scatter, top-2 axes, svd_flip signs, then the rotation (degrees), x scale and y offset of :507-520
int plateau_map(const float* pts, long long n, int mask, double angle_deg, double fx, double oy, const MapWs& w, HalfMap* m,
                long long* count, hipStream_t st) {
    const double zero[3] = {0.0, 0.0, 0.0};
    double s1[10], s2[10];
    if (int rc = moments(pts, n, mask, zero, w, s1, st)) return rc;
    const double cnt = s1[0];
    *count = (long long)cnt;
    if (*count == 0) return OAI_OK;
    const double mean[3] = {s1[1] / cnt, s1[2] / cnt, s1[3] / cnt};
    if (int rc = moments(pts, n, mask, mean, w, s2, st)) return rc;                // second pass about the mean (no cancellation)
    const double d[3] = {s2[1], s2[2], s2[3]};
    const int ij[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    double S[3][3];
    for (int k = 0; k < 6; ++k) {
        const int i = ij[k][0], j = ij[k][1];
        S[i][j] = S[j][i] = s2[4 + k] - d[i] * d[j] / cnt;
    }
    double ev[3], V[3][3];
    eig_sym3(S, ev, V);
    Axes ax;
    for (int k = 0; k < 3; ++k) ax.mean[k] = mean[k];
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 3; ++k) ax.u[c][k] = V[k][c];
    score_extreme_kernel<<<kRedBlocks, kT, 0, st>>>(pts, n, mask, ax, w.ext_partials);
    OAI_CHECK_LAUNCH();
    final_ext_kernel<<<1, kT, 0, st>>>(w.ext_partials, w.ext);
    OAI_CHECK_LAUNCH();
    Ext e[2];
    OAI_CHECK_HIP(hipMemcpyAsync(e, w.ext, sizeof(e), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < 2; ++c)
        if (e[c].v < 0.0)
            for (int k = 0; k < 3; ++k) ax.u[c][k] = -ax.u[c][k];
    const double theta = (angle_deg / 180.0) * M_PI;
    m->ax = ax;
    m->c = std::cos(theta);
    m->s = std::sin(theta);
    m->fx = fx;
    m->oy = oy;
    return OAI_OK;
}

}  // namespace

extern "C" {

size_t oai_point_grid_workspace_bytes(const int grid_dims_xyz[3], long long n_src) {
    if (!grid_dims_xyz || n_src <= 0 || grid_dims_xyz[0] <= 0 || grid_dims_xyz[1] <= 0 || grid_dims_xyz[2] <= 0) return 0;
    PointGridWs w;
    return carve(w, nullptr, (long long)grid_dims_xyz[0] * grid_dims_xyz[1] * grid_dims_xyz[2], n_src);
}

int oai_map_attributes(const float* src_pts_dev, long long n_src, const float* src_vals_dev, int n_comp, const float* tgt_pts_dev,
                       long long n_tgt, double radius, float* out_vals_dev, void* stream) {
    OAI_CHECK_ARG(src_pts_dev && src_vals_dev && tgt_pts_dev && out_vals_dev, "oai_map_attributes: null pointer");
    OAI_CHECK_ARG(n_src > 0 && n_src < (1LL << 31), "oai_map_attributes: needs 1 .. 2^31-1 source points (got %lld)", n_src);
    OAI_CHECK_ARG(n_tgt >= 0 && n_comp >= 1, "oai_map_attributes: negative target count or no point array");
    OAI_CHECK_ARG(radius >= 0.0 && std::isfinite(radius), "oai_map_attributes: radius must be finite and >= 0");
    if (n_tgt == 0) return OAI_OK;
    return launch_interp(false, src_pts_dev, n_src, src_vals_dev, n_comp, tgt_pts_dev, n_tgt, radius, UniformGrid{}, nullptr, nullptr, out_vals_dev,
                         (hipStream_t)stream);
}

int oai_map_attributes_grid(const float* src_pts_dev, long long n_src, const float* src_vals_dev, int n_comp, const float* tgt_pts_dev,
                            long long n_tgt, double radius, const double grid_lo_xyz[3], double cell_size, const int grid_dims_xyz[3],
                            void* workspace_dev, size_t workspace_bytes, float* out_vals_dev, void* stream) {
    OAI_CHECK_ARG(src_pts_dev && src_vals_dev && tgt_pts_dev && out_vals_dev && grid_lo_xyz && grid_dims_xyz && workspace_dev,
                  "oai_map_attributes_grid: null pointer");
    OAI_CHECK_ARG(n_src > 0 && n_src < (1LL << 31), "oai_map_attributes_grid: needs 1 .. 2^31-1 source points (got %lld)", n_src);
    OAI_CHECK_ARG(n_tgt >= 0 && n_comp >= 1, "oai_map_attributes_grid: negative target count or no point array");
    OAI_CHECK_ARG(radius >= 0.0 && std::isfinite(radius), "oai_map_attributes_grid: radius must be finite and >= 0");
    OAI_CHECK_ARG(cell_size > 0.0 && cell_size >= radius && std::isfinite(cell_size), "oai_map_attributes_grid: cell_size %g must be >= radius %g and > 0",
                  cell_size, radius);
    OAI_CHECK_ARG(grid_dims_xyz[0] > 0 && grid_dims_xyz[1] > 0 && grid_dims_xyz[2] > 0, "oai_map_attributes_grid: empty grid");
    const long long ncells = (long long)grid_dims_xyz[0] * grid_dims_xyz[1] * grid_dims_xyz[2];
    OAI_CHECK_ARG(ncells < (1LL << 30), "oai_map_attributes_grid: grid too fine");
    PointGridWs w;
    OAI_CHECK_WORKSPACE("oai_map_attributes_grid", workspace_bytes, carve(w, workspace_dev, ncells, n_src));
    if (n_tgt == 0) return OAI_OK;
    hipStream_t st = (hipStream_t)stream;
    const UniformGrid g = oai::make_uniform_grid(grid_lo_xyz, cell_size, grid_dims_xyz);
    if (int rc = bin_points(src_pts_dev, n_src, g, w, st)) return rc;
    return launch_interp(true, src_pts_dev, n_src, src_vals_dev, n_comp, tgt_pts_dev, n_tgt, radius, g, w.start, w.list, out_vals_dev, st);
}

int oai_point_footprint(const float* src_pts_dev, long long n_src, const float* tgt_pts_dev, long long n_tgt, double radius, int* count_dev,
                        double* nearest_d2_dev, int* nearest_j_dev, void* stream) {
    OAI_CHECK_ARG(src_pts_dev && tgt_pts_dev && count_dev && nearest_d2_dev && nearest_j_dev, "oai_point_footprint: null pointer");
    OAI_CHECK_ARG(n_src > 0 && n_src < (1LL << 31), "oai_point_footprint: needs 1 .. 2^31-1 source points (got %lld)", n_src);
    OAI_CHECK_ARG(n_tgt >= 0, "oai_point_footprint: negative target count");
    OAI_CHECK_ARG(radius >= 0.0 && std::isfinite(radius), "oai_point_footprint: radius must be finite and >= 0");
    if (n_tgt == 0) return OAI_OK;
    return launch_footprint(false, src_pts_dev, n_src, tgt_pts_dev, n_tgt, radius, UniformGrid{}, nullptr, nullptr, count_dev, nearest_d2_dev, nearest_j_dev,
                            (hipStream_t)stream);
}

int oai_point_footprint_grid(const float* src_pts_dev, long long n_src, const float* tgt_pts_dev, long long n_tgt, double radius,
                             const double grid_lo_xyz[3], double cell_size, const int grid_dims_xyz[3], void* workspace_dev, size_t workspace_bytes,
                             int* count_dev, double* nearest_d2_dev, int* nearest_j_dev, void* stream) {
    OAI_CHECK_ARG(src_pts_dev && tgt_pts_dev && count_dev && nearest_d2_dev && nearest_j_dev && grid_lo_xyz && grid_dims_xyz && workspace_dev,
                  "oai_point_footprint_grid: null pointer");
    OAI_CHECK_ARG(n_src > 0 && n_src < (1LL << 31), "oai_point_footprint_grid: needs 1 .. 2^31-1 source points (got %lld)", n_src);
    OAI_CHECK_ARG(n_tgt >= 0, "oai_point_footprint_grid: negative target count");
    OAI_CHECK_ARG(radius >= 0.0 && std::isfinite(radius), "oai_point_footprint_grid: radius must be finite and >= 0");
    OAI_CHECK_ARG(cell_size > 0.0 && cell_size >= radius && std::isfinite(cell_size), "oai_point_footprint_grid: cell_size %g must be >= radius %g and > 0",
                  cell_size, radius);
    OAI_CHECK_ARG(grid_dims_xyz[0] > 0 && grid_dims_xyz[1] > 0 && grid_dims_xyz[2] > 0, "oai_point_footprint_grid: empty grid");
    const long long ncells = (long long)grid_dims_xyz[0] * grid_dims_xyz[1] * grid_dims_xyz[2];
    OAI_CHECK_ARG(ncells < (1LL << 30), "oai_point_footprint_grid: grid too fine");
    PointGridWs w;
    OAI_CHECK_WORKSPACE("oai_point_footprint_grid", workspace_bytes, carve(w, workspace_dev, ncells, n_src));
    if (n_tgt == 0) return OAI_OK;
    hipStream_t st = (hipStream_t)stream;
    const UniformGrid g = oai::make_uniform_grid(grid_lo_xyz, cell_size, grid_dims_xyz);
    if (int rc = bin_points(src_pts_dev, n_src, g, w, st)) return rc;
    return launch_footprint(true, src_pts_dev, n_src, tgt_pts_dev, n_tgt, radius, g, w.start, w.list, count_dev, nearest_d2_dev, nearest_j_dev, st);
}

size_t oai_thickness_map_workspace_bytes(long long n_points) {
    if (n_points <= 0) return 0;
    MapWs w;
    return carve(w, nullptr, n_points);
}

int oai_fit_circle(const float* pts_dev, long long n, int col_x, int col_y, void* workspace_dev, size_t workspace_bytes, double centre_host[2],
                   double* radius_host, int* iterations_host, void* stream) {
    OAI_CHECK_ARG(pts_dev && workspace_dev && centre_host && radius_host, "oai_fit_circle: null pointer");
    OAI_CHECK_ARG(n >= 3, "oai_fit_circle: needs at least 3 points (got %lld)", n);
    OAI_CHECK_ARG(col_x >= 0 && col_x < 3 && col_y >= 0 && col_y < 3 && col_x != col_y, "oai_fit_circle: columns must be two distinct of 0, 1, 2");
    MapWs w;
    OAI_CHECK_WORKSPACE("oai_fit_circle", workspace_bytes, carve(w, workspace_dev, n));
    hipStream_t st = (hipStream_t)stream;
    // start at the centroid, as compute_least_square_circle does
    const double zero[3] = {0.0, 0.0, 0.0};
    double m[10];
    if (int rc = moments(pts_dev, n, 0, zero, w, m, st)) return rc;
    double c[2] = {m[1 + col_x] / m[0], m[1 + col_y] / m[0]};
    const double nn = (double)n;
    double S[9];
    if (int rc = circle_sums(pts_dev, n, col_x, col_y, c, w, S, st)) return rc;
    const double extent = std::sqrt(S[1] / nn);                              // rms distance of the points from their centroid
    auto cost_of = [nn](const double* s) { return s[1] - s[0] * s[0] / nn; };  // sum (R_i - mean R)^2
    double cost = cost_of(S);
    int it = 0;
    for (; it < 100; ++it) {
        // Gauss-Newton on f_i = R_i - mean R, J_i = d_i - mean d (the reference's centred Jacobian Df_2b):
        // J^T J = sum d d^T - n dbar dbar^T,  J^T f = sum d R - n dbar Rbar
        const double db0 = S[2] / nn, db1 = S[3] / nn, rb = S[0] / nn;
        const double a00 = S[4] - nn * db0 * db0, a01 = S[5] - nn * db0 * db1, a11 = S[6] - nn * db1 * db1;
        const double g0 = S[7] - nn * db0 * rb, g1 = S[8] - nn * db1 * rb;
        const double det = a00 * a11 - a01 * a01;
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) break;
        double step[2] = {-(a11 * g0 - a01 * g1) / det, -(a00 * g1 - a01 * g0) / det};
        bool accepted = false;
        double cn[2], Sn[9];
        for (int half = 0; half < 40; ++half) {                              // step halving keeps the cost from rising
            cn[0] = c[0] + step[0];
            cn[1] = c[1] + step[1];
            if (int rc = circle_sums(pts_dev, n, col_x, col_y, cn, w, Sn, st)) return rc;
            if (cost_of(Sn) <= cost) { accepted = true; break; }
            step[0] *= 0.5;
            step[1] *= 0.5;
        }
        if (!accepted) break;
        c[0] = cn[0]; c[1] = cn[1];
        for (int k = 0; k < 9; ++k) S[k] = Sn[k];
        cost = cost_of(S);
        if (std::hypot(step[0], step[1]) <= 1e-12 * extent) { ++it; break; }
    }
    centre_host[0] = c[0];
    centre_host[1] = c[1];
    *radius_host = S[0] / nn;
    if (iterations_host) *iterations_host = it;
    return OAI_OK;
}

int oai_project_circle(const float* pts_dev, long long n, int col_x, int col_y, const double centre_host[2], double* angle_dev, double* z_dev,
                       void* stream) {
    OAI_CHECK_ARG(pts_dev && centre_host && angle_dev && z_dev, "oai_project_circle: null pointer");
    OAI_CHECK_ARG(n >= 0, "oai_project_circle: negative size");
    OAI_CHECK_ARG(col_x >= 0 && col_x < 3 && col_y >= 0 && col_y < 3 && col_x != col_y, "oai_project_circle: columns must be two distinct of 0, 1, 2");
    if (n == 0) return OAI_OK;
    circle_project_kernel<<<oai::cdiv(n, kT), kT, 0, (hipStream_t)stream>>>(pts_dev, n, col_x, col_y, centre_host[0], centre_host[1], angle_dev, z_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_project_plateaus(const float* pts_dev, const float* thickness_dev, long long n, void* workspace_dev, size_t workspace_bytes,
                         double* x_dev, double* y_dev, double* thickness_out_dev, long long* n_right_host, long long* n_left_host, void* stream) {
    OAI_CHECK_ARG(pts_dev && thickness_dev && workspace_dev && x_dev && y_dev && thickness_out_dev && n_right_host && n_left_host,
                  "oai_project_plateaus: null pointer");
    OAI_CHECK_ARG(n > 0 && n < (1LL << 31), "oai_project_plateaus: needs 1 .. 2^31-1 points (got %lld)", n);
    MapWs w;
    OAI_CHECK_WORKSPACE("oai_project_plateaus", workspace_bytes, carve(w, workspace_dev, n));
    hipStream_t st = (hipStream_t)stream;
    HalfMap right, left;
    if (int rc = plateau_map(pts_dev, n, 2, -160.0, -1.0, 50.0, w, &right, n_right_host, st)) return rc;
    if (int rc = plateau_map(pts_dev, n, 1, -50.0, 1.0, 0.0, w, &left, n_left_host, st)) return rc;
    if (*n_right_host == 0 || *n_left_host == 0)
        return oai::set_error(OAI_ERR_ARG, "oai_project_plateaus: the %s plateau is empty (no point with z %s 50)", *n_right_host == 0 ? "right" : "left",
                              *n_right_host == 0 ? ">=" : "<");
    half_flags_kernel<<<oai::cdiv(n + 1, kT), kT, 0, st>>>(pts_dev, n, w.right, w.left);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.right, w.off_right, n + 1, w.scratch, st)) return rc;
    if (int rc = oai::exclusive_scan_i32(w.left, w.off_left, n + 1, w.scratch, st)) return rc;
    plateau_project_kernel<<<oai::cdiv(n, kT), kT, 0, st>>>(pts_dev, thickness_dev, n, right, left, w.off_right, w.off_left, *n_right_host, x_dev,
                                                            y_dev, thickness_out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
