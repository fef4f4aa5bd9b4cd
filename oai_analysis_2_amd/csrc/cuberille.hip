// Cuberille iso-surface for gfx950: get_mesh_from_probability_map (oai_analysis/mesh_processing.py:343-350) on the device.
//
// The reference calls itk.cuberille_image_to_mesh_filter(image, generate_triangle_faces=True, iso_surface_value=0.5,
// project_vertices_to_iso_surface=True, project_vertex_surface_distance_threshold=0.05).  ITK is not installed here, so the filter
// is restated (unpinned); the contract is in include/oai_hip.h.  In short: one quad per (inside voxel, outside face
// neighbour) pair, voxels in raster order and neighbours in the order -z -y -x +x +y +z; one vertex per lattice point a face uses,
// numbered in order of first use; vertices then walked to the iso-surface along the interpolated gradient.
//
//   oai_cuberille_count   classify (6-bit outside-neighbour mask per voxel) -> scan of the face counts -> atomicMin of the first
//                         corner slot 4 f + q of every lattice point -> per voxel the number of slots that are their point's first
//                         use -> scan: the vertex ids in first-use order, whatever order the atomics ran in
//   oai_cuberille_emit    vertex ids per lattice point -> faces (two triangles or one quad per face) -> one thread per vertex: the
//                         physical point and the projection loop in fp64
//
// Everything but the projection is a handful of streaming passes over the volume and the (D+1)(H+1)(W+1) lattice.  The projection
// gathers 8 voxels for the value and 48 for the gradient per step from L2.  No float atomics and no contraction: the bits equal the
// numpy restatement (tests/cuberille_ref.py) on every run.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kT = 256;

struct Geo {                      // the physical geometry and the projection settings, by value
    double o[3], s[3], d[9], m[9];  // origin, spacing (x, y, z), direction and inv(direction diag(spacing)), row-major
    double iso, thr, step0, relax;
    int max_steps, move_after, project;
    int D, H, W;
};

// lattice point of corner q of face j of voxel (x, y, z): j = 0..5 is -z -y -x +x +y +z; the face on axis a has in-plane axes
// (b, c) = cyclic successors of a, corners (0,0) (1,0) (1,1) (0,1) on the + side and (0,0) (0,1) (1,1) (1,0) on the - side
__device__ __forceinline__ int corner_lattice(int x, int y, int z, int j, int q, int H, int W) {
    const int a = j < 3 ? 2 - j : j - 3;
    const bool plus = j >= 3;
    int v[3] = {x, y, z};
    v[a] += plus ? 1 : 0;
    const int ob = plus ? (q == 1 || q == 2) : (q == 2 || q == 3);
    const int oc = plus ? (q == 2 || q == 3) : (q == 1 || q == 2);
    v[(a + 1) % 3] += ob;
    v[(a + 2) % 3] += oc;
    return (v[2] * (H + 1) + v[1]) * (W + 1) + v[0];
}

__device__ __forceinline__ void voxel_xyz(long long i, int H, int W, int& x, int& y, int& z) {
    x = (int)(i % W);
    y = (int)((i / W) % H);
    z = (int)(i / ((long long)W * H));
}

// mask[i] = bit j set: voxel i is inside (value >= iso) and its neighbour j is outside (or off the grid); cnt[i] = popcount, cnt[n] = 0
__global__ void __launch_bounds__(kT) cub_classify_kernel(const float* __restrict__ vol, int D, int H, int W, float iso,
                                                          unsigned char* __restrict__ mask, int* __restrict__ cnt) {
    const long long n = (long long)D * H * W;
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    if (i == n) { cnt[n] = 0; return; }
    int x, y, z;
    voxel_xyz(i, H, W, x, y, z);
    const long long sy = W, sz = (long long)W * H;
    unsigned m = 0;
    if (vol[i] >= iso) {
        if (z == 0 || !(vol[i - sz] >= iso)) m |= 1u;
        if (y == 0 || !(vol[i - sy] >= iso)) m |= 2u;
        if (x == 0 || !(vol[i - 1] >= iso)) m |= 4u;
        if (x == W - 1 || !(vol[i + 1] >= iso)) m |= 8u;
        if (y == H - 1 || !(vol[i + sy] >= iso)) m |= 16u;
        if (z == D - 1 || !(vol[i + sz] >= iso)) m |= 32u;
    }
    mask[i] = (unsigned char)m;
    cnt[i] = __popc(m);
}

// first[L] = min over the corner slots 4 f + q that use lattice point L
__global__ void __launch_bounds__(kT) cub_first_use_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ foff, long long n,
                                                           int H, int W, int* __restrict__ first) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const unsigned m = mask[i];
    if (!m) return;
    int x, y, z;
    voxel_xyz(i, H, W, x, y, z);
    int f = foff[i];
    for (int j = 0; j < 6; ++j) {
        if (!(m & (1u << j))) continue;
        for (int q = 0; q < 4; ++q) atomicMin(&first[corner_lattice(x, y, z, j, q, H, W)], 4 * f + q);
        ++f;
    }
}

// nv[i] = the corner slots of voxel i that are the first use of their lattice point; nv[n] = 0
__global__ void __launch_bounds__(kT) cub_new_count_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ foff, long long n,
                                                           int H, int W, const int* __restrict__ first, int* __restrict__ nv) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    if (i == n) { nv[n] = 0; return; }
    const unsigned m = mask[i];
    int c = 0;
    if (m) {
        int x, y, z;
        voxel_xyz(i, H, W, x, y, z);
        int f = foff[i];
        for (int j = 0; j < 6; ++j) {
            if (!(m & (1u << j))) continue;
            for (int q = 0; q < 4; ++q) c += first[corner_lattice(x, y, z, j, q, H, W)] == 4 * f + q;
            ++f;
        }
    }
    nv[i] = c;
}

// vid[L] = the vertex id of every used lattice point; verts[3 id] temporarily holds L (read back by cub_vertex_kernel)
__global__ void __launch_bounds__(kT) cub_vertex_ids_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ foff,
                                                            const int* __restrict__ voff, long long n, int H, int W, const int* __restrict__ first,
                                                            int* __restrict__ vid, long long nv_cap, int* __restrict__ stash) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const unsigned m = mask[i];
    if (!m) return;
    int x, y, z;
    voxel_xyz(i, H, W, x, y, z);
    int f = foff[i], id = voff[i];
    for (int j = 0; j < 6; ++j) {
        if (!(m & (1u << j))) continue;
        for (int q = 0; q < 4; ++q) {
            const int L = corner_lattice(x, y, z, j, q, H, W);
            if (first[L] == 4 * f + q) {
                vid[L] = id;
                if (id >= 0 && id < nv_cap) stash[3 * (long long)id] = L;
                ++id;
            }
        }
        ++f;
    }
}

__global__ void __launch_bounds__(kT) cub_faces_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ foff, long long n, int H, int W,
                                                       const int* __restrict__ vid, int triangles, int flip, long long nf_cap, int* __restrict__ faces) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const unsigned m = mask[i];
    if (!m) return;
    int x, y, z;
    voxel_xyz(i, H, W, x, y, z);
    long long f = foff[i];
    for (int j = 0; j < 6; ++j) {
        if (!(m & (1u << j))) continue;
        int c[4];
        for (int q = 0; q < 4; ++q) c[q] = vid[corner_lattice(x, y, z, j, q, H, W)];
        if (f >= 0 && f < nf_cap) {
            if (triangles) {                 // (q0 q1 q2) (q0 q2 q3); flipped: each triangle's last two swapped
                int* t = faces + 6 * f;
                t[0] = c[0]; t[1] = flip ? c[2] : c[1]; t[2] = flip ? c[1] : c[2];
                t[3] = c[0]; t[4] = flip ? c[3] : c[2]; t[5] = flip ? c[2] : c[3];
            } else {                         // (q0 q1 q2 q3); flipped: (q0 q3 q2 q1)
                int* t = faces + 4 * f;
                t[0] = c[0]; t[1] = flip ? c[3] : c[1]; t[2] = c[2]; t[3] = flip ? c[1] : c[3];
            }
        }
        ++f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// projection (fp64, numpy's operation order, no contraction)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    return a + t * (b - a);
}

__device__ __forceinline__ double vox(const float* __restrict__ vol, int x, int y, int z, int H, int W) {
    return (double)vol[((long long)z * H + y) * W + x];
}

// value and index-space gradient (central differences, replicated borders, divided by 2 s) interpolated trilinearly at the continuous
// index c (clamped to [0, n-1]); the gradient is returned rotated by the direction
__device__ void sample(const float* __restrict__ vol, const Geo& g, const double c[3], double& val, double grad[3]) {
#pragma clang fp contract(off)
    const int n[3] = {g.W, g.H, g.D};
    int i0[3], i1[3];
    double t[3];
    for (int k = 0; k < 3; ++k) {
        const double hi = (double)(n[k] - 1);
        const double cc = c[k] < 0.0 ? 0.0 : (c[k] > hi ? hi : c[k]);
        int a = (int)floor(cc);
        if (a > n[k] - 2) a = n[k] - 2;
        if (a < 0) a = 0;
        i0[k] = a;
        i1[k] = a + 1 < n[k] ? a + 1 : n[k] - 1;
        t[k] = cc - (double)a;
    }
    double v[8], gx[8], gy[8], gz[8];
    for (int corner = 0; corner < 8; ++corner) {        // corner bit 0: x, bit 1: y, bit 2: z
        const int x = corner & 1 ? i1[0] : i0[0], y = corner & 2 ? i1[1] : i0[1], z = corner & 4 ? i1[2] : i0[2];
        v[corner] = vox(vol, x, y, z, g.H, g.W);
        const int xm = x > 0 ? x - 1 : 0, xp = x + 1 < g.W ? x + 1 : g.W - 1;
        const int ym = y > 0 ? y - 1 : 0, yp = y + 1 < g.H ? y + 1 : g.H - 1;
        const int zm = z > 0 ? z - 1 : 0, zp = z + 1 < g.D ? z + 1 : g.D - 1;
        gx[corner] = (vox(vol, xp, y, z, g.H, g.W) - vox(vol, xm, y, z, g.H, g.W)) / (2.0 * g.s[0]);
        gy[corner] = (vox(vol, x, yp, z, g.H, g.W) - vox(vol, x, ym, z, g.H, g.W)) / (2.0 * g.s[1]);
        gz[corner] = (vox(vol, x, y, zp, g.H, g.W) - vox(vol, x, y, zm, g.H, g.W)) / (2.0 * g.s[2]);
    }
    auto tri = [&](const double* f) {
        const double a = lerp(f[0], f[1], t[0]), b = lerp(f[2], f[3], t[0]), cc = lerp(f[4], f[5], t[0]), d = lerp(f[6], f[7], t[0]);
        return lerp(lerp(a, b, t[1]), lerp(cc, d, t[1]), t[2]);
    };
    val = tri(v);
    const double gi[3] = {tri(gx), tri(gy), tri(gz)};
    for (int r = 0; r < 3; ++r) grad[r] = (g.d[3 * r] * gi[0] + g.d[3 * r + 1] * gi[1]) + g.d[3 * r + 2] * gi[2];
}

__global__ void __launch_bounds__(kT) cub_vertex_kernel(const float* __restrict__ vol, Geo g, const int* __restrict__ voff, long long n,
                                                        long long nv_cap, float* __restrict__ verts, int* __restrict__ steps) {
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    const long long nv = voff[n] < nv_cap ? voff[n] : nv_cap;
    if (v >= nv) return;
    const int L = reinterpret_cast<const int*>(verts)[3 * v];
    const int li = L % (g.W + 1), lj = (L / (g.W + 1)) % (g.H + 1), lk = L / ((g.W + 1) * (g.H + 1));
    const double u[3] = {g.s[0] * ((double)li - 0.5), g.s[1] * ((double)lj - 0.5), g.s[2] * ((double)lk - 0.5)};
    double p[3];
    for (int r = 0; r < 3; ++r) p[r] = g.o[r] + ((g.d[3 * r] * u[0] + g.d[3 * r + 1] * u[1]) + g.d[3 * r + 2] * u[2]);
    int k = 0;
    if (g.project) {
        double step = g.step0;
        for (;;) {
            const double e[3] = {p[0] - g.o[0], p[1] - g.o[1], p[2] - g.o[2]};
            double c[3];
            for (int r = 0; r < 3; ++r) c[r] = (g.m[3 * r] * e[0] + g.m[3 * r + 1] * e[1]) + g.m[3 * r + 2] * e[2];
            double val, gr[3];
            sample(vol, g, c, val, gr);
            const double len = sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
            if (len == 0.0) break;
            const double m = val - g.iso;
            bool done = fabs(m) <= g.thr;
            if (done && !g.move_after) break;
            const double s = m < 0.0 ? step : -step;
            for (int r = 0; r < 3; ++r) p[r] = p[r] + s * (gr[r] / len);
            ++k;
            done = done || k > g.max_steps;
            step = step * g.relax;
            if (done) break;
        }
    }
    for (int r = 0; r < 3; ++r) verts[3 * v + r] = (float)p[r];
    if (steps) steps[v] = k;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Workspaces: one struct of typed pointers per entry-point family, filled by one carve() that returns the bytes walked (oai::Ws,
// common.h): over a null base that is the *_workspace_bytes answer, over the caller's buffer the carving.
struct CubWs { unsigned char* mask; int *foff, *voff, *first, *vid, *scratch; };
size_t carve(CubWs& w, const void* base, long long n, long long lattice) {
    oai::Ws ws(base);
    w.mask = ws.take<unsigned char>(n);
    w.foff = ws.take<int>(n + 1);
    w.voff = ws.take<int>(n + 1);
    w.first = ws.take<int>(lattice);
    w.vid = ws.take<int>(lattice);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(n + 1) / 4);
    return ws.off;
}

long long lattice_points(int D, int H, int W) { return (long long)(D + 1) * (H + 1) * (W + 1); }

// every corner slot 4 f + q (f < 3 n + 2 (HW + DW + DH): one face per neighbour pair or border face) and every lattice index fit an int
bool size_ok(int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return false;
    const long long n = (long long)D * H * W;
    const long long max_faces = 3 * n + 2 * ((long long)H * W + (long long)D * W + (long long)D * H);
    return 4 * max_faces < INT_MAX && lattice_points(D, H, W) < INT_MAX;
}

}  // namespace

extern "C" {

size_t oai_cuberille_workspace_bytes(int D, int H, int W) {
    if (!size_ok(D, H, W)) return 0;
    CubWs w;
    return carve(w, nullptr, (long long)D * H * W, lattice_points(D, H, W));
}

int oai_cuberille_count(const float* vol_dev, int D, int H, int W, float iso, void* workspace_dev, size_t workspace_bytes,
                        long long* n_verts, long long* n_faces, void* stream) {
    OAI_CHECK_ARG(vol_dev && workspace_dev && n_verts && n_faces, "oai_cuberille_count: null pointer");
    OAI_CHECK_ARG(D >= 1 && H >= 1 && W >= 1, "oai_cuberille_count: every axis needs at least 1 voxel (got %d x %d x %d)", D, H, W);
    OAI_CHECK_ARG(size_ok(D, H, W), "oai_cuberille_count: volume %d x %d x %d too large for 32-bit corner slots", D, H, W);
    OAI_CHECK_ARG(!std::isnan(iso), "oai_cuberille_count: iso value is NaN");
    const long long n = (long long)D * H * W, lat = lattice_points(D, H, W);
    CubWs w;
    OAI_CHECK_WORKSPACE("oai_cuberille_count", workspace_bytes, carve(w, workspace_dev, n, lat));
    hipStream_t st = (hipStream_t)stream;
    cub_classify_kernel<<<oai::cdiv(n + 1, kT), kT, 0, st>>>(vol_dev, D, H, W, iso, w.mask, w.foff);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.foff, w.foff, n + 1, w.scratch, st)) return rc;
    OAI_CHECK_HIP(hipMemsetAsync(w.first, 0x7f, (size_t)lat * 4, st));        // 0x7f7f7f7f > every corner slot
    cub_first_use_kernel<<<oai::cdiv(n, kT), kT, 0, st>>>(w.mask, w.foff, n, H, W, w.first);
    OAI_CHECK_LAUNCH();
    cub_new_count_kernel<<<oai::cdiv(n + 1, kT), kT, 0, st>>>(w.mask, w.foff, n, H, W, w.first, w.voff);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.voff, w.voff, n + 1, w.scratch, st)) return rc;
    int tot[2];                                                 // the caller sizes its output arrays from the counts
    if (int rc = oai::read_ints(tot, {w.voff + n, w.foff + n}, st)) return rc;
    *n_verts = tot[0];
    *n_faces = tot[1];
    return OAI_OK;
}

int oai_cuberille_emit(const float* vol_dev, int D, int H, int W, float iso, const double geometry_host[24], int flip_winding, int triangles,
                       int project, double threshold, double step_length, double relaxation, int max_steps, int move_after_converged,
                       void* workspace_dev, size_t workspace_bytes, long long n_verts, long long n_faces, float* verts_dev, int* faces_dev,
                       int* steps_dev, void* stream) {
    OAI_CHECK_ARG(vol_dev && geometry_host && workspace_dev && verts_dev && faces_dev, "oai_cuberille_emit: null pointer");
    OAI_CHECK_ARG(D >= 1 && H >= 1 && W >= 1, "oai_cuberille_emit: every axis needs at least 1 voxel (got %d x %d x %d)", D, H, W);
    OAI_CHECK_ARG(size_ok(D, H, W), "oai_cuberille_emit: volume %d x %d x %d too large for 32-bit corner slots", D, H, W);
    OAI_CHECK_ARG(n_verts >= 0 && n_faces >= 0, "oai_cuberille_emit: negative vertex or face count");
    const long long n = (long long)D * H * W, lat = lattice_points(D, H, W);
    CubWs w;
    OAI_CHECK_WORKSPACE("oai_cuberille_emit", workspace_bytes, carve(w, workspace_dev, n, lat));
    Geo g;
    for (int k = 0; k < 3; ++k) { g.o[k] = geometry_host[k]; g.s[k] = geometry_host[3 + k]; }
    for (int k = 0; k < 9; ++k) { g.d[k] = geometry_host[6 + k]; g.m[k] = geometry_host[15 + k]; }
    bool finite = true;
    for (int k = 0; k < 24; ++k) finite = finite && std::isfinite(geometry_host[k]);
    OAI_CHECK_ARG(finite, "oai_cuberille_emit: the geometry holds a non-finite value");
    OAI_CHECK_ARG(g.s[0] > 0.0 && g.s[1] > 0.0 && g.s[2] > 0.0, "oai_cuberille_emit: spacing must be positive");
    if (project) {
        OAI_CHECK_ARG(threshold >= 0.0 && std::isfinite(threshold), "oai_cuberille_emit: threshold must be finite and >= 0");
        OAI_CHECK_ARG(relaxation > 0.0 && std::isfinite(relaxation), "oai_cuberille_emit: relaxation factor must be finite and > 0");
        OAI_CHECK_ARG(max_steps >= 0, "oai_cuberille_emit: max_steps must be >= 0 (got %d)", max_steps);
        OAI_CHECK_ARG(std::isfinite(step_length), "oai_cuberille_emit: step length is not finite");
    }
    const double smax = g.s[0] > g.s[1] ? (g.s[0] > g.s[2] ? g.s[0] : g.s[2]) : (g.s[1] > g.s[2] ? g.s[1] : g.s[2]);
    g.iso = (double)iso;
    g.thr = threshold;
    g.step0 = step_length < 0.0 ? 0.25 * smax : step_length;
    g.relax = relaxation;
    g.max_steps = max_steps;
    g.move_after = move_after_converged ? 1 : 0;
    g.project = project ? 1 : 0;
    g.D = D; g.H = H; g.W = W;
    hipStream_t st = (hipStream_t)stream;
    if (n_verts > 0 || n_faces > 0) {
        cub_vertex_ids_kernel<<<oai::cdiv(n, kT), kT, 0, st>>>(w.mask, w.foff, w.voff, n, H, W, w.first, w.vid, n_verts, reinterpret_cast<int*>(verts_dev));
        OAI_CHECK_LAUNCH();
    }
    if (n_faces > 0) {
        cub_faces_kernel<<<oai::cdiv(n, kT), kT, 0, st>>>(w.mask, w.foff, n, H, W, w.vid, triangles ? 1 : 0, flip_winding ? 1 : 0, n_faces, faces_dev);
        OAI_CHECK_LAUNCH();
    }
    if (n_verts > 0) {
        cub_vertex_kernel<<<oai::cdiv(n_verts, kT), kT, 0, st>>>(vol_dev, g, w.voff, n, n_verts, verts_dev, steps_dev);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

}  // extern "C"
