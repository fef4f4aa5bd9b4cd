// Cartilage morphometry for gfx950 (include/oai_hip.h, "Cartilage morphometry"; tests/morphometry_ref.py restates this file operation
// for operation): what turns the per-vertex thickness of csrc/thickness_map.hip into the figures a study tabulates.
//   oai_mesh_areas     per-face area and per-vertex area (a third of the incident faces' areas) of a triangle mesh
//   oai_region_stats   per region, the twelve area-weighted and unweighted sums behind mean thickness, covered and denuded area
// (the third primitive, oai_point_footprint, sits beside the kernels whose binning it shares, in csrc/thickness_map.hip).
//
// fp64 without contraction.  The order IS the contract.  A vertex adds its corners' face areas in ascending corner index (3 f + k: face
// index, then corner): the vertex-to-corner incidence is built by count -> exclusive scan -> scatter with integer atomics, which decide
// slots and never a sum, and each vertex then walks its own short list smallest corner first.  The region sums follow
// csrc/ordered_reduce.h with the thread layout of surface_partials_kernel (csrc/edt.hip).  No floating-point atomics.
//
// Gather- and latency-bound VALU work on <= 10^5 elements: one element per thread or a grid-stride walk, no LDS beyond the block reduction.
#include "common.h"

#include <cmath>

#include "ordered_reduce.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr long long kStreamBlocks = 2048;          // surface_partials_kernel's cap: grid-stride beyond that
constexpr int kRS = 12;                            // doubles per region of oai_region_stats
constexpr int kMaxRegions = 64;

// ---- oai_mesh_areas ------------------------------------------------------------------------------------------------------------------
// one thread per face: its area, and one count per corner at the vertex the corner names
__global__ void __launch_bounds__(kT) face_area_kernel(const float* __restrict__ verts, long long n, const int* __restrict__ faces, long long m,
                                                       double* __restrict__ area, int* __restrict__ count) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    if (f >= m) return;
    const int* c = faces + 3 * f;
    if (!face_ok(c, n)) { area[f] = (double)NAN; return; }      // not a triangle of this mesh: no area, incident to no vertex
    const float *a = verts + 3 * (long long)c[0], *b = verts + 3 * (long long)c[1], *d = verts + 3 * (long long)c[2];
    const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
    const double e2x = (double)d[0] - (double)a[0], e2y = (double)d[1] - (double)a[1], e2z = (double)d[2] - (double)a[2];
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    for (int k = 0; k < 3; ++k) atomicAdd(&count[c[k]], 1);
}

// one thread per corner: a slot in its vertex's list (the order inside a list is whatever the atomics gave; vertex_area_kernel sorts it out)
__global__ void __launch_bounds__(kT) corner_scatter_kernel(const int* __restrict__ faces, long long n, long long m, const int* __restrict__ start,
                                                            int* __restrict__ cursor, int* __restrict__ corners) {
    const long long c = (long long)blockIdx.x * kT + threadIdx.x;
    if (c >= 3 * m) return;
    if (!face_ok(faces + 3 * (c / 3), n)) return;
    const int v = faces[c];
    corners[start[v] + atomicAdd(&cursor[v], 1)] = (int)c;
}

// one thread per vertex: its corners in ascending index (they are distinct: each step takes the smallest one above the last), O(degree^2)
__global__ void __launch_bounds__(kT) vertex_area_kernel(const int* __restrict__ start, const int* __restrict__ corners, const double* __restrict__ area,
                                                         long long n, double* __restrict__ vertex_area) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n) return;
    const int s = start[v], e = start[v + 1];
    double sum = 0.0;
    int last = -1;
    for (int t = s; t < e; ++t) {
        int next = 0x7fffffff;
        for (int k = s; k < e; ++k) {
            const int c = corners[k];
            if (c > last && c < next) next = c;
        }
        sum = sum + area[next / 3];
        last = next;
    }
    vertex_area[v] = sum / 3.0;
}

struct AreaWs {
    double* area;
    int *count, *start, *corners, *scratch;
    size_t bytes;
    AreaWs(void* workspace, long long n, long long m) {
        Ws ws(workspace);
        area = ws.take<double>((size_t)m);
        count = ws.take<int>((size_t)n + 1);
        start = ws.take<int>((size_t)n + 1);
        corners = ws.take<int>((size_t)(3 * m));
        scratch = ws.take<int>(scan_scratch_bytes(n + 1) / 4);
        bytes = ws.off;
    }
};

// ---- oai_region_stats ----------------------------------------------------------------------------------------------------------------
struct RegionAcc {
    double v[kRS];       // elements, covered, measured, sum w (all, covered, measured), sum w t, sum (w t) t, min t, max t, sum t, sum t t
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < kRS; ++i) v[i] = 0.0;
        v[8] = INFINITY; v[9] = -INFINITY;
    }
    __device__ __forceinline__ void merge(const double* o) {       // this (the earlier elements) on the left of every operation
#pragma unroll
        for (int i = 0; i < kRS; ++i) v[i] = i == 8 ? fmin(v[i], o[i]) : (i == 9 ? fmax(v[i], o[i]) : v[i] + o[i]);
    }
};

// grid (blocks, n_regions): block (b, r) walks the whole array in surface_partials_kernel's layout and touches only region r's elements
__global__ void __launch_bounds__(kT)
region_partials_kernel(const float* __restrict__ values, const double* __restrict__ weights, const int* __restrict__ labels,
                       const unsigned char* __restrict__ covered, long long n, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kRS];
    const int r = blockIdx.y;
    RegionAcc acc;
    acc.clear();
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        if ((labels ? labels[i] : 0) != r) continue;
        const float f = values[i];
        const double w = weights[i], t = (double)f;
        acc.v[0] = acc.v[0] + 1.0; acc.v[3] = acc.v[3] + w;
        if (covered && !covered[i]) continue;
        acc.v[1] = acc.v[1] + 1.0; acc.v[4] = acc.v[4] + w;
        if (!finite_f32(f)) continue;
        const double wt = w * t;
        acc.v[2] = acc.v[2] + 1.0; acc.v[5] = acc.v[5] + w; acc.v[6] = acc.v[6] + wt; acc.v[7] = acc.v[7] + wt * t;
        acc.v[8] = fmin(acc.v[8], t); acc.v[9] = fmax(acc.v[9], t);
        acc.v[10] = acc.v[10] + t; acc.v[11] = acc.v[11] + t * t;
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kRS; ++i) partials[((long long)r * gridDim.x + blockIdx.x) * kRS + i] = acc.v[i];
}

// one block per region: its slots in the order of csrc/ordered_reduce.h
__global__ void __launch_bounds__(kT) region_finish_kernel(const double* __restrict__ partials, long long nb, double* __restrict__ out) {
    __shared__ double lds[kT / 64][kRS];
    RegionAcc acc;
    reduce_slots<kT>(partials + (long long)blockIdx.x * nb * kRS, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kRS; ++i) out[(long long)blockIdx.x * kRS + i] = acc.v[i];
}

struct RegionWs {
    double* partials;
    long long blocks;
    size_t bytes;
    RegionWs(void* workspace, long long n, int n_regions) {
        Ws ws(workspace);
        blocks = (long long)grid_stride_blocks(n, kT * 4, kStreamBlocks);
        partials = ws.take<double>((size_t)blocks * n_regions * kRS);
        bytes = ws.off;
    }
};

}  // namespace

extern "C" {

size_t oai_mesh_areas_workspace_bytes(long long n_verts, long long n_faces) {
    if (!mesh_ok(n_verts, n_faces)) return 0;
    return AreaWs(nullptr, n_verts, n_faces).bytes;
}

int oai_mesh_areas(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, void* workspace_dev, size_t workspace_bytes,
                   double* face_area_dev, double* vertex_area_dev, void* stream) {
    OAI_CHECK_ARG(mesh_ok(n_verts, n_faces), "oai_mesh_areas: needs 0 .. 2^31-2 vertices and 0 .. 2^28 faces (got %lld, %lld)", n_verts, n_faces);
    OAI_CHECK_ARG(workspace_dev && (n_verts == 0 || (verts_dev && vertex_area_dev)) && (n_faces == 0 || faces_dev), "oai_mesh_areas: null pointer");
    OAI_CHECK_WORKSPACE("oai_mesh_areas", workspace_bytes, oai_mesh_areas_workspace_bytes(n_verts, n_faces));
    const AreaWs ws(workspace_dev, n_verts, n_faces);
    const hipStream_t st = (hipStream_t)stream;
    double* area = face_area_dev ? face_area_dev : ws.area;
    if (int rc = bucket_clear(ws.count, n_verts, st)) return rc;
    if (n_faces) {
        face_area_kernel<<<cdiv(n_faces, kT), kT, 0, st>>>(verts_dev, n_verts, faces_dev, n_faces, area, ws.count);
        OAI_CHECK_LAUNCH();
    }
    if (n_verts == 0) return OAI_OK;
    if (int rc = bucket_starts(ws.count, ws.start, n_verts, ws.scratch, st)) return rc;
    if (n_faces) {
        corner_scatter_kernel<<<cdiv(3 * n_faces, kT), kT, 0, st>>>(faces_dev, n_verts, n_faces, ws.start, ws.count, ws.corners);
        OAI_CHECK_LAUNCH();
    }
    vertex_area_kernel<<<cdiv(n_verts, kT), kT, 0, st>>>(ws.start, ws.corners, area, n_verts, vertex_area_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_region_stats_workspace_bytes(long long n, int n_regions) {
    if (n < 0 || n_regions < 1 || n_regions > kMaxRegions) return 0;
    return RegionWs(nullptr, n, n_regions).bytes;
}

int oai_region_stats(const float* values_dev, const double* weights_dev, const int* labels_dev, const unsigned char* covered_dev, long long n,
                     int n_regions, void* workspace_dev, size_t workspace_bytes, double* out_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_region_stats: negative element count (%lld)", n);
    OAI_CHECK_ARG(n_regions >= 1 && n_regions <= kMaxRegions, "oai_region_stats: n_regions must be in [1, %d], got %d", kMaxRegions, n_regions);
    OAI_CHECK_ARG(out_dev && workspace_dev && (n == 0 || (values_dev && weights_dev)), "oai_region_stats: null pointer");
    OAI_CHECK_WORKSPACE("oai_region_stats", workspace_bytes, oai_region_stats_workspace_bytes(n, n_regions));
    const RegionWs ws(workspace_dev, n, n_regions);
    const hipStream_t st = (hipStream_t)stream;
    region_partials_kernel<<<dim3((unsigned)ws.blocks, (unsigned)n_regions), kT, 0, st>>>(values_dev, weights_dev, labels_dev, covered_dev, n, ws.partials);
    OAI_CHECK_LAUNCH();
    region_finish_kernel<<<n_regions, kT, 0, st>>>(ws.partials, ws.blocks, out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
