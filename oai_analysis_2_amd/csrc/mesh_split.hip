// Inner / outer split of a cartilage surface for gfx950: split_mesh (oai_analysis/mesh_processing.py:197-294, 353-378) on the device.
//
// The reference clusters per-face features with scikit-learn KMeans(n_clusters=2, algorithm="lloyd") on the host:
//   TC: features [cn, 10 n] (6 columns), one fit with n_init = 1 (sklearn >= 1.4: n_init="auto" is one run for k-means++)
//   FC: features [cn, n, (bbox centre - c) * n] (9 columns), the faces cut into three x slabs of cn, one fit per slab with n_init = 5
// with c the face centroid, n the unit face normal and cn = (c - mean c) / (max c - min c) per axis.  Everything here restates
// sklearn 1.7's _kmeans.py (fit, _kmeans_plusplus, _kmeans_single_lloyd) in fp64:
//   oai_mesh_split_features  centroid / normal per face (bit-identical to the numpy helpers), the exact sequential column sums of
//                            the centroids (numpy's axis-0 mean adds row after row), min / max, slab membership, and each slab's
//                            feature columns compacted (SoA, ascending face index).  Returns the slab sizes: the host draws the
//                            random numbers of every fit from them (RandomState(5).choice / uniform, exactly as sklearn does).
//   oai_mesh_split_kmeans    ONE launch, one workgroup per (slab, init) run: centring, k-means++ seeding with 2 local trials,
//                            the whole Lloyd loop (at most max_iter), the final E-step and the inertia.  Then one workgroup per
//                            slab applies fit()'s best-of-init rule (_is_same_clustering) and the orientation (:212-217).
//   oai_mesh_submesh         get_vtk_sub_mesh (:150-194): the selected faces in ascending order, the vertices in order of first
//                            use in the flattened face list (integer atomicMin of the position: order-independent), remapped.
// One workgroup per run rather than a multi-workgroup Lloyd step: a slab is at most a few MB of features, the 15 FC runs already
// occupy 15 CUs at once, and a launch per iteration would cost more than a pass over a slab from L2.
//
// Reductions are fixed-order (per thread a fixed stride, a fixed shuffle tree per wave, the waves in order): no float atomics, the
// same bits on every run.  Labels can differ from sklearn's only where a face is within rounding of equidistant from both centres
// (sklearn's distances come from BLAS).  An empty cluster (sklearn relocates a point there) cannot arise from a non-degenerate mesh;
// it is reported as an error instead of being restated.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kT = 256;              // threads of the per-face kernels
constexpr int kRT = 512;             // threads of a k-means run / slab selection workgroup (8 waves: 256 VGPRs, no spills)
constexpr int kWaves = kRT / 64;
constexpr int kRedBlocks = 256;      // blocks of the min / max reduction
constexpr int kMaxSlabs = 3;         // FC: num_divisions = 3 (:245)
constexpr int kMaxInit = 5;          // FC: n_init = 5 (:231)
constexpr int kMaxRuns = kMaxSlabs * kMaxInit;
constexpr int kMaxD = 9;
constexpr int kSumTile = 4096;       // rows staged per step of the sequential column sum

// ---------------------------------------------------------------------------------------------------------------------
// per-face attributes and features (numpy's operation order, no contraction)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) face_attr_kernel(const float* __restrict__ verts, long long n_verts, const int* __restrict__ faces,
                                                       long long n_faces, double* __restrict__ cent, double* __restrict__ nrm,
                                                       int* __restrict__ bad_index) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n_faces) return;
    int idx[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * i + k];
        ok = ok && idx[k] >= 0 && idx[k] < n_verts;
    }
    if (!ok) {
        atomicOr(bad_index, 1);
        for (int k = 0; k < 3; ++k) cent[3 * i + k] = nrm[3 * i + k] = NAN;
        return;
    }
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)verts[3 * (long long)idx[0] + k];
        b[k] = (double)verts[3 * (long long)idx[1] + k];
        c[k] = (double)verts[3 * (long long)idx[2] + k];
    }
    for (int k = 0; k < 3; ++k) cent[3 * i + k] = ((a[k] + b[k]) + c[k]) / 3.0;          // v[faces].sum(axis=1) / 3.0
    double u[3], w[3];
    for (int k = 0; k < 3; ++k) { u[k] = b[k] - a[k]; w[k] = c[k] - a[k]; }
    const double x = u[1] * w[2] - u[2] * w[1], y = u[2] * w[0] - u[0] * w[2], z = u[0] * w[1] - u[1] * w[0];      // np.cross
    const double len = sqrt((x * x + y * y) + z * z);                                                               // np.linalg.norm
    const double d = len > 0.0 ? len : 1.0;
    nrm[3 * i] = x / d;
    nrm[3 * i + 1] = y / d;
    nrm[3 * i + 2] = z / d;
}

// np.mean(c, axis=0): numpy adds the rows one after another.  The block stages kSumTile rows, three lanes add them in order.
__global__ void __launch_bounds__(kRT) col_sum_seq_kernel(const double* __restrict__ cent, long long n, double* __restrict__ sum_out) {
    __shared__ double tile[kSumTile * 3];
    double s = 0.0;
    for (long long r0 = 0; r0 < n; r0 += kSumTile) {
        const int rows = (int)(n - r0 < kSumTile ? n - r0 : kSumTile);
        __syncthreads();
        for (int k = threadIdx.x; k < 3 * rows; k += kRT) tile[k] = cent[3 * r0 + k];
        __syncthreads();
        if (threadIdx.x < 3) {
            int r = 0;
            for (; r + 16 <= rows; r += 16) {           // the 16 LDS reads issue ahead of the dependent adds, which stay in row order
                double t[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) t[j] = tile[3 * (r + j) + threadIdx.x];
#pragma unroll
                for (int j = 0; j < 16; ++j) s += t[j];
            }
            for (; r < rows; ++r) s += tile[3 * r + threadIdx.x];
        }
    }
    if (threadIdx.x < 3) sum_out[threadIdx.x] = s;
}

// min / max of the centroids (fp64) and of the vertices (float32): exact in any order
struct MinMax {
    double cmin[3], cmax[3];
    float vmin[3], vmax[3];
};

__device__ __forceinline__ void mm_init(MinMax& m) {
    for (int k = 0; k < 3; ++k) { m.cmin[k] = INFINITY; m.cmax[k] = -INFINITY; m.vmin[k] = INFINITY; m.vmax[k] = -INFINITY; }
}

__device__ __forceinline__ void mm_merge(MinMax& m, const MinMax& o) {
    for (int k = 0; k < 3; ++k) {
        m.cmin[k] = fmin(m.cmin[k], o.cmin[k]); m.cmax[k] = fmax(m.cmax[k], o.cmax[k]);
        m.vmin[k] = fminf(m.vmin[k], o.vmin[k]); m.vmax[k] = fmaxf(m.vmax[k], o.vmax[k]);
    }
}

__device__ __forceinline__ void mm_block_store(MinMax& m, MinMax* __restrict__ dst) {
    __shared__ MinMax sh[kT];
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) mm_merge(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = sh[0];
}

__global__ void __launch_bounds__(kT) minmax_kernel(const double* __restrict__ cent, long long n_faces, const float* __restrict__ verts,
                                                    long long n_verts, MinMax* __restrict__ partials) {
    MinMax m;
    mm_init(m);
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n_faces; i += (long long)kRedBlocks * kT)
        for (int k = 0; k < 3; ++k) { m.cmin[k] = fmin(m.cmin[k], cent[3 * i + k]); m.cmax[k] = fmax(m.cmax[k], cent[3 * i + k]); }
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n_verts; i += (long long)kRedBlocks * kT)
        for (int k = 0; k < 3; ++k) { m.vmin[k] = fminf(m.vmin[k], verts[3 * i + k]); m.vmax[k] = fmaxf(m.vmax[k], verts[3 * i + k]); }
    mm_block_store(m, partials + blockIdx.x);
}

__global__ void __launch_bounds__(kT) minmax_final_kernel(const MinMax* __restrict__ partials, MinMax* __restrict__ out) {
    MinMax m;
    mm_init(m);
    if ((int)threadIdx.x < kRedBlocks) m = partials[threadIdx.x];
    mm_block_store(m, out);
}

struct Stats {
    double csum[3];
    MinMax mm;
};

// per face: the normalised centroid cn, the features of its fit and the slabs it lies in (numpy's order of operations)
struct FaceFeat {
    double f[kMaxD];
    int mask;                // bit s: the face is in slab s
};

__device__ __forceinline__ FaceFeat face_features(const double* __restrict__ cent, const double* __restrict__ nrm, long long i, long long n,
                                                  const Stats& st, int fc) {
#pragma clang fp contract(off)
    FaceFeat r;
    double cn[3], mean[3], range[3];
    for (int k = 0; k < 3; ++k) {
        mean[k] = st.csum[k] / (double)n;
        range[k] = st.mm.cmax[k] - st.mm.cmin[k];
        cn[k] = (cent[3 * i + k] - mean[k]) / range[k];
        r.f[k] = cn[k];
    }
    if (!fc) {
        for (int k = 0; k < 3; ++k) r.f[3 + k] = nrm[3 * i + k] * 10.0;
        r.mask = 1;
        return r;
    }
    for (int k = 0; k < 3; ++k) {
        // centre = (bbox_min + bbox_max) / 2 of the mesh's float32 bounds, in float32 (Mesh.GetBounds gives float32 scalars)
        const float centre = (st.mm.vmin[k] + st.mm.vmax[k]) / 2.0f;
        r.f[3 + k] = nrm[3 * i + k];
        r.f[6 + k] = ((double)centre - cent[3 * i + k]) * nrm[3 * i + k];
    }
    // the slabs of :259-270: min / max of cn_x are the images of min / max c_x (x -> (x - m) / r rounds monotonically for r > 0)
    const double min_x = (st.mm.cmin[0] - mean[0]) / range[0], max_x = (st.mm.cmax[0] - mean[0]) / range[0];
    const double step = (max_x - min_x) / 3.0;
    r.mask = 0;
    for (int s = 0; s < kMaxSlabs; ++s) {
        const double lower = min_x + step * (double)s, upper = lower + step;
        if (cn[0] >= lower && cn[0] < upper) r.mask |= 1 << s;       // rounding can leave a face in no slab or (at a seam) in two
    }
    return r;
}

// flags[s][i] = face i lies in slab s; flags[s][n] = 0 so that the scans end on the slab sizes
__global__ void __launch_bounds__(kT) slab_flags_kernel(const double* __restrict__ cent, const double* __restrict__ nrm, long long n,
                                                        const Stats* __restrict__ stats, int fc, int n_slabs, int* __restrict__ flags,
                                                        signed char* __restrict__ mask_out) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    const int mask = i < n ? face_features(cent, nrm, i, n, *stats, fc).mask : 0;
    if (i < n) mask_out[i] = (signed char)mask;
    for (int s = 0; s < n_slabs; ++s) flags[s * (n + 1) + i] = (mask >> s) & 1;
}

// each slab's feature columns, compacted in ascending face order: slab s, column k at feat[off_s * D + k * n_s + p]
__global__ void __launch_bounds__(kT) compact_kernel(const double* __restrict__ cent, const double* __restrict__ nrm, long long n,
                                                     const Stats* __restrict__ stats, int fc, int n_slabs, int d, const int* __restrict__ pos,
                                                     double* __restrict__ feat, int* __restrict__ face_of) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const FaceFeat ff = face_features(cent, nrm, i, n, *stats, fc);
    long long off = 0;
    for (int s = 0; s < n_slabs; ++s) {
        const long long ns = pos[s * (n + 1) + n];
        if ((ff.mask >> s) & 1) {
            const long long p = pos[s * (n + 1) + i];
            for (int k = 0; k < d; ++k) feat[off * d + k * ns + p] = ff.f[k];
            face_of[off + p] = (int)i;
        }
        off += ns;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k-means: one workgroup per (slab, init) run
// ---------------------------------------------------------------------------------------------------------------------
struct KParams {
    long long n[kMaxSlabs], off[kMaxSlabs];
    long long first[kMaxRuns];      // rs.choice(n, p=w / w.sum()) of each run
    double u[kMaxRuns][2];          // rs.uniform(size=2) of each run
    long long stride;               // elements between two inits' label / distance arrays
    int n_slabs, n_init, max_iter;
};

struct RunOut {
    double inertia;
    double centre[2][kMaxD];        // in centred coordinates
    int n_iter;
    int status;                     // 1: a cluster became empty
};

struct SlabOut {
    int best, n_iter, flipped, status;
};

// K sums over the workgroup in a fixed order; every thread gets the totals.  sh: (kWaves + 1) * K doubles
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
    __syncthreads();
    if ((int)threadIdx.x < K) {
        double s = sh[threadIdx.x];
        for (int w = 1; w < kWaves; ++w) s += sh[w * K + threadIdx.x];
        sh[kWaves * K + threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[kWaves * K + k];
    __syncthreads();
}

template <int K>
__device__ __forceinline__ void block_min(long long (&v)[K], long long* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] = min(v[k], (long long)__shfl_xor(v[k], o, 64));
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        long long m = sh[k];
        for (int w = 1; w < kWaves; ++w) m = min(m, sh[w * K + k]);
        v[k] = m;
    }
    __syncthreads();
}

// exclusive prefix of one value per thread over the workgroup (fixed order), and the total
__device__ __forceinline__ double block_excl_scan(double v, double* sh, double* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double incl = v;
    for (int dd = 1; dd < 64; dd <<= 1) {
        const double o = __shfl_up(incl, dd, 64);
        if (lane >= dd) incl += o;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    double woff = 0.0, tot = 0.0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) woff += sh[w];
        tot += sh[w];
    }
    __syncthreads();
    *total = tot;
    return woff + (incl - v);
}

template <int D>
__device__ __forceinline__ double dot(const double (&x)[D], const double (&c)[D]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s += x[k] * c[k];
    return s;
}

template <int D>
__device__ __forceinline__ double sqnorm(const double (&x)[D]) { return dot<D>(x, x); }

// _euclidean_distances(c, X, Y_norm_squared=xx, squared=True): max(-2 x.c + |c|^2 + |x|^2, 0)
template <int D>
__device__ __forceinline__ double sqdist_expanded(const double (&x)[D], double xx, const double (&c)[D], double cc) {
    return fmax((-2.0 * dot<D>(x, c) + cc) + xx, 0.0);
}

template <int D>
__global__ void __launch_bounds__(kRT) kmeans_run_kernel(const double* __restrict__ feat, KParams p, double tol_factor,
                                                         signed char* __restrict__ labels_all, double* __restrict__ dist_all,
                                                         RunOut* __restrict__ out) {
    __shared__ double sh[(kWaves + 1) * (2 * D + 3)];
    const int run = blockIdx.x, s = run / p.n_init, r = run % p.n_init;
    const long long n = p.n[s];
    const double* __restrict__ X = feat + p.off[s] * D;
    signed char* __restrict__ lab = labels_all + r * p.stride + p.off[s];
    double* __restrict__ dist = dist_all + r * p.stride + p.off[s];
    auto raw = [&](long long i, double (&x)[D]) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = X[k * n + i];
    };

    // fit(): X -= X.mean(axis=0); tol = mean(var(X, axis=0)) * 1e-4
    double mean[D];
    {
        double v[D];
        for (int k = 0; k < D; ++k) v[k] = 0.0;
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            raw(i, x);
            for (int k = 0; k < D; ++k) v[k] += x[k];
        }
        block_sum<D>(v, sh);
        for (int k = 0; k < D; ++k) mean[k] = v[k] / (double)n;
    }
    auto load = [&](long long i, double (&x)[D]) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = X[k * n + i] - mean[k];
    };
    double tol;
    {
        double v[D];
        for (int k = 0; k < D; ++k) v[k] = 0.0;
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            load(i, x);
            for (int k = 0; k < D; ++k) v[k] += x[k] * x[k];
        }
        block_sum<D>(v, sh);
        double m = 0.0;
        for (int k = 0; k < D; ++k) m += v[k] / (double)n;
        tol = m / D * tol_factor;
    }

    // _kmeans_plusplus with n_local_trials = 2 + int(log(2)) = 2
    double c[2][D], cn[2][D];
    load(p.first[run], c[0]);
    double cc0 = sqnorm<D>(c[0]);
    double pot;
    {
        double v[1] = {0.0};
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            load(i, x);
            const double d = sqdist_expanded<D>(x, sqnorm<D>(x), c[0], cc0);
            dist[i] = d;
            v[0] += d;
        }
        block_sum<1>(v, sh);
        pot = v[0];
    }
    long long cand[2];
    {
        const double rv[2] = {p.u[run][0] * pot, p.u[run][1] * pot};
        long long first_ge[2] = {LLONG_MAX, LLONG_MAX};
        double base = 0.0;
        __syncthreads();                        // the distances of this workgroup are visible to all its threads
        for (long long t0 = 0; t0 < n; t0 += 4 * kRT) {
            const long long i0 = t0 + 4 * (long long)threadIdx.x;
            double v[4];
            for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? dist[i0 + j] : 0.0;
            double total;
            double run_sum = base + block_excl_scan(((v[0] + v[1]) + v[2]) + v[3], sh, &total);
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= n) break;
                run_sum += v[j];                // the cumulative sum through element i0 + j
                for (int t = 0; t < 2; ++t)
                    if (run_sum >= rv[t] && i0 + j < first_ge[t]) first_ge[t] = i0 + j;
            }
            base += total;
        }
        block_min<2>(first_ge, (long long*)sh);
        for (int t = 0; t < 2; ++t) cand[t] = first_ge[t] < n - 1 ? first_ge[t] : n - 1;     // searchsorted, clipped to n - 1
    }
    {
        load(cand[0], cn[0]);
        load(cand[1], cn[1]);
        const double ca = sqnorm<D>(cn[0]), cb = sqnorm<D>(cn[1]);
        double v[2] = {0.0, 0.0};
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            load(i, x);
            const double xx = sqnorm<D>(x), d = dist[i];
            v[0] += fmin(d, sqdist_expanded<D>(x, xx, cn[0], ca));
            v[1] += fmin(d, sqdist_expanded<D>(x, xx, cn[1], cb));
        }
        block_sum<2>(v, sh);
        const int b = v[1] < v[0] ? 1 : 0;     // argmin: the first on a tie
        for (int k = 0; k < D; ++k) c[1][k] = cn[b][k];
    }

    // _kmeans_single_lloyd
    int it = 0, status = 0;
    bool strict = false;
    for (; it < p.max_iter; ++it) {
        const double q0 = sqnorm<D>(c[0]), q1 = sqnorm<D>(c[1]);
        double v[2 * D + 3];
        for (int k = 0; k < 2 * D + 3; ++k) v[k] = 0.0;
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            load(i, x);
            const double d0 = q0 + (-2.0 * dot<D>(x, c[0])), d1 = q1 + (-2.0 * dot<D>(x, c[1]));
            const int l = d1 < d0 ? 1 : 0;
            if (it > 0 && lab[i] != l) v[2 * D + 2] += 1.0;
            lab[i] = (signed char)l;
            if (l) {
                for (int k = 0; k < D; ++k) v[D + k] += x[k];
                v[2 * D + 1] += 1.0;
            } else {
                for (int k = 0; k < D; ++k) v[k] += x[k];
                v[2 * D] += 1.0;
            }
        }
        block_sum<2 * D + 3>(v, sh);
        if (v[2 * D] == 0.0 || v[2 * D + 1] == 0.0) { status = 1; break; }
        double shift_tot = 0.0;
        for (int j = 0; j < 2; ++j) {
            const double alpha = 1.0 / v[2 * D + j];                    // _average_centers
            double sh2 = 0.0;
            for (int k = 0; k < D; ++k) {
                const double nc = v[j * D + k] * alpha, dd = nc - c[j][k];
                sh2 += dd * dd;
                c[j][k] = nc;
            }
            const double shift = sqrt(sh2);                              // _center_shift, then (center_shift ** 2).sum()
            shift_tot += shift * shift;
        }
        if (it > 0 && v[2 * D + 2] == 0.0) { strict = true; break; }   // labels equal to the previous iteration's
        if (shift_tot <= tol) break;
    }
    const int n_iter = it + 1 < p.max_iter ? it + 1 : p.max_iter;
    double inertia = 0.0;
    if (!status) {
        const double q0 = sqnorm<D>(c[0]), q1 = sqnorm<D>(c[1]);
        double v[1] = {0.0};
        for (long long i = threadIdx.x; i < n; i += kRT) {
            double x[D];
            load(i, x);
            int l;
            if (strict) {
                l = lab[i];
            } else {                                                     // the E-step on the final centres
                const double d0 = q0 + (-2.0 * dot<D>(x, c[0])), d1 = q1 + (-2.0 * dot<D>(x, c[1]));
                l = d1 < d0 ? 1 : 0;
                lab[i] = (signed char)l;
            }
            double e = 0.0;
            for (int k = 0; k < D; ++k) {
                const double dd = x[k] - (l ? c[1][k] : c[0][k]);
                e += dd * dd;
            }
            v[0] += e;
        }
        block_sum<1>(v, sh);
        inertia = v[0];
    }
    if (threadIdx.x == 0) {
        RunOut o;
        o.inertia = inertia;
        for (int j = 0; j < 2; ++j)
            for (int k = 0; k < kMaxD; ++k) o.centre[j][k] = k < D ? c[j][k] : 0.0;
        o.n_iter = n_iter;
        o.status = status;
        out[run] = o;
    }
}

// fit()'s choice among the inits (run i replaces the best only if its inertia is smaller AND its labels are not the best's up to a
// relabelling), then the orientation: side = 2 label - 1, all flipped if the mean n_y over side -1 is negative.  A face in two slabs
// takes the later slab's side (np.put in slab order).
__global__ void __launch_bounds__(kRT) select_orient_kernel(const RunOut* __restrict__ runs, KParams p, const signed char* __restrict__ labels_all,
                                                            const int* __restrict__ face_of, const signed char* __restrict__ slab_mask,
                                                            const double* __restrict__ nrm, signed char* __restrict__ side, SlabOut* __restrict__ out) {
    __shared__ double sh[(kWaves + 1) * 2];
    const int s = blockIdx.x;
    const long long n = p.n[s], off = p.off[s];
    auto lab = [&](int r) { return labels_all + r * p.stride + off; };
    for (int r = 0; r < p.n_init; ++r)
        if (runs[s * p.n_init + r].status) {
            if (threadIdx.x == 0) out[s] = SlabOut{-1, 0, 0, 1};
            return;
        }
    int best = 0;
    for (int r = 1; r < p.n_init; ++r) {
        if (!(runs[s * p.n_init + r].inertia < runs[s * p.n_init + best].inertia)) continue;
        // _is_same_clustering(labels_r, labels_best): mapping[a] = labels_best at the first i with labels_r == a, then every i agrees
        const signed char* __restrict__ lr = lab(r);
        const signed char* __restrict__ lb = lab(best);
        long long first[2] = {LLONG_MAX, LLONG_MAX};
        for (long long i = threadIdx.x; i < n; i += kRT) {
            const int a = lr[i];
            if (i < first[a]) first[a] = i;
        }
        block_min<2>(first, (long long*)sh);
        const int m0 = first[0] < n ? lb[first[0]] : -1, m1 = first[1] < n ? lb[first[1]] : -1;
        double v[1] = {0.0};
        for (long long i = threadIdx.x; i < n; i += kRT)
            if (lb[i] != (lr[i] ? m1 : m0)) v[0] += 1.0;
        block_sum<1>(v, sh);
        if (v[0] != 0.0) best = r;
    }
    const signed char* __restrict__ lb = lab(best);
    double v[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < n; i += kRT)
        if (lb[i] == 0) {
            v[0] += nrm[3 * (long long)face_of[off + i] + 1];
            v[1] += 1.0;
        }
    block_sum<2>(v, sh);
    const bool flip = v[1] > 0.0 && v[0] / v[1] < 0.0;      // an empty side -1 has a NaN mean: no flip
    for (long long i = threadIdx.x; i < n; i += kRT) {
        const int f = face_of[off + i];
        if (slab_mask[f] >> (s + 1)) continue;              // a later slab holds this face too and writes it
        const int sd = 2 * lb[i] - 1;
        side[f] = (signed char)(flip ? -sd : sd);
    }
    if (threadIdx.x == 0) out[s] = SlabOut{best, runs[s * p.n_init + best].n_iter, flip ? 1 : 0, 0};
}

// ---------------------------------------------------------------------------------------------------------------------
// sub-mesh extraction (get_vtk_sub_mesh)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) select_flags_kernel(const signed char* __restrict__ side, long long n, int which, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && side[i] == which;
}

__global__ void __launch_bounds__(kT) first_use_kernel(const int* __restrict__ faces, long long n_faces, long long n_verts,
                                                       const int* __restrict__ flag, const int* __restrict__ fpos, int* __restrict__ first,
                                                       int* __restrict__ face_idx_out, int* __restrict__ bad_index) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n_faces || !flag[i]) return;
    const int q = fpos[i];
    face_idx_out[q] = (int)i;
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * i + k];
        if (v < 0 || v >= n_verts) { atomicOr(bad_index, 1); continue; }
        atomicMin(&first[v], 3 * q + k);
    }
}

// occ[p] = the flattened position p is its vertex's first use; occ[3 m] = 0
__global__ void __launch_bounds__(kT) first_flags_kernel(const int* __restrict__ faces, long long n_verts, const int* __restrict__ face_idx,
                                                         long long m, const int* __restrict__ first, int* __restrict__ occ) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p > 3 * m) return;
    int o = 0;
    if (p < 3 * m) {
        const int v = faces[3 * (long long)face_idx[p / 3] + p % 3];
        o = v >= 0 && v < n_verts && first[v] == (int)p;
    }
    occ[p] = o;
}

__global__ void __launch_bounds__(kT) submesh_scatter_kernel(const float* __restrict__ verts, long long n_verts, const int* __restrict__ faces,
                                                             const int* __restrict__ face_idx, long long m, const int* __restrict__ first,
                                                             const int* __restrict__ occ, const int* __restrict__ rank, float* __restrict__ verts_out,
                                                             int* __restrict__ faces_out) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p >= 3 * m) return;
    const int v = faces[3 * (long long)face_idx[p / 3] + p % 3];
    if (v < 0 || v >= n_verts) { faces_out[p] = -1; return; }
    if (occ[p]) {
        const long long o = rank[p];
        for (int k = 0; k < 3; ++k) verts_out[3 * o + k] = verts[3 * (long long)v + k];
    }
    faces_out[p] = rank[first[v]];
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int slabs_of(int mesh_type) { return mesh_type == OAI_MESH_FC ? kMaxSlabs : 1; }
int dims_of(int mesh_type) { return mesh_type == OAI_MESH_FC ? 9 : 6; }

// compacted slab rows: every face at most once, plus room for the faces that rounding puts in two neighbouring FC slabs (a face
// exactly at a seam; oai_mesh_split_features refuses a mesh with more of them than this)
long long slab_capacity(long long n_faces, int mesh_type) { return mesh_type == OAI_MESH_FC ? n_faces + n_faces / 64 + 64 : n_faces; }

// Workspaces: one struct of typed pointers per entry-point family, filled by one carve() that returns the bytes walked (oai::Ws,
// common.h): over a null base that is the *_workspace_bytes answer, over the caller's buffer the carving.
// The features part first, the per-run part (labels, distances: one row set per init) last, so that the features call needs only
// the bytes of n_init = 1.
struct SplitWs {
    Stats* stats; MinMax* partials; int* bad; signed char* mask; int *flags, *pos; double* feat; int* face_of; RunOut* runs; SlabOut* slabs;
    int* scratch; signed char* labels; double* dist;
    long long cap;
};
size_t carve(SplitWs& w, const void* base, long long n_faces, int mesh_type, int n_init) {
    const int S = slabs_of(mesh_type), D = dims_of(mesh_type);
    oai::Ws ws(base);
    w.cap = slab_capacity(n_faces, mesh_type);
    w.stats = ws.take<Stats>(1);
    w.partials = ws.take<MinMax>(kRedBlocks);
    w.bad = ws.take<int>(1);
    w.mask = ws.take<signed char>(n_faces);
    w.flags = ws.take<int>((size_t)S * (n_faces + 1));
    w.pos = ws.take<int>((size_t)S * (n_faces + 1));
    w.feat = ws.take<double>((size_t)w.cap * D);
    w.face_of = ws.take<int>(w.cap);
    w.runs = ws.take<RunOut>(kMaxRuns);
    w.slabs = ws.take<SlabOut>(kMaxSlabs);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(n_faces + 1) / 4);
    w.labels = ws.take<signed char>((size_t)n_init * w.cap);
    w.dist = ws.take<double>((size_t)n_init * w.cap);
    return ws.off;
}

struct SubWs { int *flag, *fpos, *first, *occ, *rank, *bad, *scratch; };
size_t carve(SubWs& w, const void* base, long long n_verts, long long n_faces) {
    oai::Ws ws(base);
    w.flag = ws.take<int>(n_faces + 1);
    w.fpos = ws.take<int>(n_faces + 1);
    w.first = ws.take<int>(n_verts);
    w.occ = ws.take<int>(3 * n_faces + 1);
    w.rank = ws.take<int>(3 * n_faces + 1);
    w.bad = ws.take<int>(1);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(3 * n_faces + 1) / 4);
    return ws.off;
}

using oai::kMaxFaces;

bool valid_type(int t) { return t == OAI_MESH_FC || t == OAI_MESH_TC; }

}  // namespace

extern "C" {

size_t oai_mesh_split_workspace_bytes(long long n_verts, long long n_faces, int mesh_type, int n_init) {
    if (n_verts <= 0 || n_faces < 2 || n_faces >= kMaxFaces || !valid_type(mesh_type) || n_init < 1 || n_init > kMaxInit) return 0;
    SplitWs w;
    return carve(w, nullptr, n_faces, mesh_type, n_init);
}

int oai_mesh_split_features(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, int mesh_type,
                            void* workspace_dev, size_t workspace_bytes, double* centroids_dev, double* normals_dev,
                            long long slab_counts_host[3], void* stream) {
    OAI_CHECK_ARG(verts_dev && faces_dev && workspace_dev && centroids_dev && normals_dev && slab_counts_host,
                  "oai_mesh_split_features: null pointer");
    OAI_CHECK_ARG(valid_type(mesh_type), "oai_mesh_split_features: mesh_type must be OAI_MESH_FC (0) or OAI_MESH_TC (1), got %d", mesh_type);
    OAI_CHECK_ARG(n_faces >= 2 && n_faces < kMaxFaces, "oai_mesh_split_features: needs 2 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_verts >= 3 && n_verts < (1LL << 31), "oai_mesh_split_features: needs 3 .. 2^31-1 vertices (got %lld)", n_verts);
    SplitWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_split_features", workspace_bytes, carve(w, workspace_dev, n_faces, mesh_type, 1));
    hipStream_t st = (hipStream_t)stream;
    const int S = slabs_of(mesh_type), D = dims_of(mesh_type), fc = mesh_type == OAI_MESH_FC;
    Stats* stats = w.stats;
    int *bad = w.bad, *flags = w.flags, *pos = w.pos;
    OAI_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    face_attr_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(verts_dev, n_verts, faces_dev, n_faces, centroids_dev, normals_dev, bad);
    OAI_CHECK_LAUNCH();
    col_sum_seq_kernel<<<1, kRT, 0, st>>>(centroids_dev, n_faces, stats->csum);
    OAI_CHECK_LAUNCH();
    minmax_kernel<<<kRedBlocks, kT, 0, st>>>(centroids_dev, n_faces, verts_dev, n_verts, w.partials);
    OAI_CHECK_LAUNCH();
    minmax_final_kernel<<<1, kT, 0, st>>>(w.partials, &stats->mm);
    OAI_CHECK_LAUNCH();
    slab_flags_kernel<<<oai::cdiv(n_faces + 1, kT), kT, 0, st>>>(centroids_dev, normals_dev, n_faces, stats, fc, S, flags, w.mask);
    OAI_CHECK_LAUNCH();
    for (int s = 0; s < S; ++s)
        if (int rc = oai::exclusive_scan_i32(flags + s * (n_faces + 1), pos + s * (n_faces + 1), n_faces + 1, w.scratch, st)) return rc;
    int counts[kMaxSlabs] = {0, 0, 0}, bad_host = 0;
    Stats st_host;
    for (int s = 0; s < S; ++s)
        OAI_CHECK_HIP(hipMemcpyAsync(&counts[s], pos + s * (n_faces + 1) + n_faces, sizeof(int), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipMemcpyAsync(&bad_host, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipMemcpyAsync(&st_host, stats, sizeof(Stats), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    if (bad_host) return oai::set_error(OAI_ERR_ARG, "oai_mesh_split_features: a face indexes outside the %lld vertices", n_verts);
    for (int k = 0; k < 3; ++k)
        if (!(st_host.mm.cmax[k] - st_host.mm.cmin[k] > 0.0) || !std::isfinite(st_host.mm.cmax[k] - st_host.mm.cmin[k]) || !std::isfinite(st_host.csum[k]))
            return oai::set_error(OAI_ERR_ARG, "oai_mesh_split_features: the centroids have no finite, non-zero extent along axis %d", k);
    long long total = 0;
    for (int s = 0; s < S; ++s) total += counts[s];
    if (total > w.cap)
        return oai::set_error(OAI_ERR_ARG, "oai_mesh_split_features: %lld faces lie on a seam of two slabs (room for %lld)", total - n_faces,
                              w.cap - n_faces);
    compact_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(centroids_dev, normals_dev, n_faces, stats, fc, S, D, pos, w.feat, w.face_of);
    OAI_CHECK_LAUNCH();
    for (int s = 0; s < kMaxSlabs; ++s) slab_counts_host[s] = s < S ? counts[s] : 0;
    return OAI_OK;
}

int oai_mesh_split_kmeans(long long n_faces, int mesh_type, void* workspace_dev, size_t workspace_bytes, const double* normals_dev, int n_init,
                          int max_iter, const long long slab_counts_host[3], const long long* first_centre_host, const double* uniforms_host,
                          signed char* side_dev, int* n_iter_host, void* stream) {
    OAI_CHECK_ARG(workspace_dev && normals_dev && slab_counts_host && first_centre_host && uniforms_host && side_dev && n_iter_host,
                  "oai_mesh_split_kmeans: null pointer");
    OAI_CHECK_ARG(valid_type(mesh_type), "oai_mesh_split_kmeans: mesh_type must be OAI_MESH_FC (0) or OAI_MESH_TC (1), got %d", mesh_type);
    OAI_CHECK_ARG(n_faces >= 2 && n_faces < kMaxFaces, "oai_mesh_split_kmeans: needs 2 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_init >= 1 && n_init <= kMaxInit, "oai_mesh_split_kmeans: n_init must be 1 .. %d (got %d)", kMaxInit, n_init);
    OAI_CHECK_ARG(max_iter >= 1, "oai_mesh_split_kmeans: max_iter must be >= 1 (got %d)", max_iter);
    SplitWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_split_kmeans", workspace_bytes, carve(w, workspace_dev, n_faces, mesh_type, n_init));
    const int S = slabs_of(mesh_type), D = dims_of(mesh_type);
    KParams p{};
    long long off = 0;
    for (int s = 0; s < S; ++s) {
        const long long ns = slab_counts_host[s];
        OAI_CHECK_ARG(ns >= 2 && ns <= n_faces, "oai_mesh_split_kmeans: slab %d has %lld faces: n_samples=%lld should be >= n_clusters=2", s, ns, ns);
        p.n[s] = ns;
        p.off[s] = off;
        off += ns;
    }
    OAI_CHECK_ARG(off <= w.cap, "oai_mesh_split_kmeans: the slab sizes add up to %lld > %lld", off, w.cap);
    for (int r = 0; r < S * n_init; ++r) {
        const int s = r / n_init;
        OAI_CHECK_ARG(first_centre_host[r] >= 0 && first_centre_host[r] < p.n[s], "oai_mesh_split_kmeans: first centre %lld of run %d is outside slab %d",
                      first_centre_host[r], r, s);
        OAI_CHECK_ARG(uniforms_host[2 * r] >= 0.0 && uniforms_host[2 * r] < 1.0 && uniforms_host[2 * r + 1] >= 0.0 && uniforms_host[2 * r + 1] < 1.0,
                      "oai_mesh_split_kmeans: uniforms of run %d are not in [0, 1)", r);
        p.first[r] = first_centre_host[r];
        p.u[r][0] = uniforms_host[2 * r];
        p.u[r][1] = uniforms_host[2 * r + 1];
    }
    p.stride = w.cap;
    p.n_slabs = S;
    p.n_init = n_init;
    p.max_iter = max_iter;
    hipStream_t st = (hipStream_t)stream;
    OAI_CHECK_HIP(hipMemsetAsync(side_dev, 0, (size_t)n_faces, st));
    if (D == 9)
        kmeans_run_kernel<9><<<S * n_init, kRT, 0, st>>>(w.feat, p, 1e-4, w.labels, w.dist, w.runs);
    else
        kmeans_run_kernel<6><<<S * n_init, kRT, 0, st>>>(w.feat, p, 1e-4, w.labels, w.dist, w.runs);
    OAI_CHECK_LAUNCH();
    select_orient_kernel<<<S, kRT, 0, st>>>(w.runs, p, w.labels, w.face_of, w.mask, normals_dev, side_dev, w.slabs);
    OAI_CHECK_LAUNCH();
    SlabOut so[kMaxSlabs];
    OAI_CHECK_HIP(hipMemcpyAsync(so, w.slabs, S * sizeof(SlabOut), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < S; ++s) {
        if (so[s].status)
            return oai::set_error(OAI_ERR_ARG, "oai_mesh_split_kmeans: a cluster of slab %d became empty during Lloyd iterations (sklearn would "
                                               "relocate a point; not restated here)", s);
        n_iter_host[s] = so[s].n_iter;
    }
    return OAI_OK;
}

size_t oai_mesh_submesh_workspace_bytes(long long n_verts, long long n_faces) {
    if (n_verts <= 0 || n_faces <= 0 || n_faces >= kMaxFaces || n_verts >= (1LL << 31)) return 0;
    SubWs w;
    return carve(w, nullptr, n_verts, n_faces);
}

int oai_mesh_submesh(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const signed char* side_dev, int which,
                     void* workspace_dev, size_t workspace_bytes, float* verts_out_dev, int* faces_out_dev, int* face_idx_out_dev,
                     long long* n_verts_out_host, long long* n_faces_out_host, void* stream) {
    OAI_CHECK_ARG(verts_dev && faces_dev && side_dev && workspace_dev && verts_out_dev && faces_out_dev && face_idx_out_dev && n_verts_out_host &&
                      n_faces_out_host, "oai_mesh_submesh: null pointer");
    OAI_CHECK_ARG(n_faces >= 1 && n_faces < kMaxFaces, "oai_mesh_submesh: needs 1 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_verts >= 1 && n_verts < (1LL << 31), "oai_mesh_submesh: needs 1 .. 2^31-1 vertices (got %lld)", n_verts);
    OAI_CHECK_ARG(which >= -128 && which <= 127, "oai_mesh_submesh: side value %d is not an int8", which);
    SubWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_submesh", workspace_bytes, carve(w, workspace_dev, n_verts, n_faces));
    hipStream_t st = (hipStream_t)stream;
    select_flags_kernel<<<oai::cdiv(n_faces + 1, kT), kT, 0, st>>>(side_dev, n_faces, which, w.flag);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.flag, w.fpos, n_faces + 1, w.scratch, st)) return rc;
    OAI_CHECK_HIP(hipMemsetAsync(w.first, 0x7f, (size_t)n_verts * 4, st));        // 0x7f7f7f7f > every flattened position
    OAI_CHECK_HIP(hipMemsetAsync(w.bad, 0, sizeof(int), st));
    first_use_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces_dev, n_faces, n_verts, w.flag, w.fpos, w.first, face_idx_out_dev, w.bad);
    OAI_CHECK_LAUNCH();
    int h[2];                                                                     // selected faces, bad-index flag
    if (int rc = oai::read_ints(h, {w.fpos + n_faces, w.bad}, st)) return rc;
    if (h[1]) return oai::set_error(OAI_ERR_ARG, "oai_mesh_submesh: a face indexes outside the %lld vertices", n_verts);
    const int m = h[0];
    *n_faces_out_host = m;
    *n_verts_out_host = 0;
    if (m == 0) return OAI_OK;
    const long long np = 3LL * m;
    first_flags_kernel<<<oai::cdiv(np + 1, kT), kT, 0, st>>>(faces_dev, n_verts, face_idx_out_dev, m, w.first, w.occ);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.occ, w.rank, np + 1, w.scratch, st)) return rc;
    submesh_scatter_kernel<<<oai::cdiv(np, kT), kT, 0, st>>>(verts_dev, n_verts, faces_dev, face_idx_out_dev, m, w.first, w.occ, w.rank, verts_out_dev,
                                                            faces_out_dev);
    OAI_CHECK_LAUNCH();
    int nv = 0;
    if (int rc = oai::read_ints(&nv, {w.rank + np}, st)) return rc;
    *n_verts_out_host = nv;
    return OAI_OK;
}

}  // extern "C"
