// Iso-surface + smoothing + closest-point distance for gfx950: the step after the hot path.
//
// Replaces, on the device, the three library calls of oai_analysis/mesh_processing.py:
//   skimage.measure.marching_cubes(img, level=0.5, spacing, step_size=1)      (:325-336)  -> oai_mc_count / oai_mc_emit
//   vtkSmoothPolyDataFilter(num_iterations=150)                                 (:298-307)  -> oai_mesh_smooth
//   vtkDistancePolyDataFilter(SignedDistanceOff, ComputeSecondDistance)         (:310-322)  -> oai_mesh_point_distance
// None of skimage / vtk is installed, so the published algorithms are restated (see oracle/mesh.py for the conventions):
// marching cubes with a case table generated from first principles (face-consistent, watertight), Jacobi Laplacian
// smoothing over the edge graph, exact closest point on a triangle (Ericson 5.1.5).
//
// All three are HBM / VALU streaming kernels; nothing here is GEMM-shaped.
#include "common.h"
#include "uniform_grid.h"

#include <mutex>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// case table, generated on the host (same construction as oracle/mesh.py: tests compare the two tables entry by entry)
// ---------------------------------------------------------------------------------------------------------------------
const int kFaces[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};   // ccw seen from outside

int edge_of(int c0, int c1) {
    const int d = c0 ^ c1, lo = c0 < c1 ? c0 : c1;
    const int x = lo & 1, y = (lo >> 1) & 1, z = lo >> 2;
    if (d == 1) return 0 * 4 + y + 2 * z;
    if (d == 2) return 1 * 4 + x + 2 * z;
    return 2 * 4 + x + 2 * y;
}

// do two cube edges lie on a common cube face?  edge = axis * 4 + j, j's two bits = the coordinates along the other two axes
bool share_face(int e1, int e2) {
    auto faces = [](int e, int (&f)[2]) {
        const int axis = e >> 2, j = e & 3;
        const int o0 = axis == 0 ? 1 : 0, o1 = axis == 2 ? 1 : 2;
        f[0] = o0 * 2 + (j & 1);
        f[1] = o1 * 2 + (j >> 1);
    };
    int a[2], b[2];
    faces(e1, a);
    faces(e2, b);
    return a[0] == b[0] || a[0] == b[1] || a[1] == b[0] || a[1] == b[1];
}

struct Tables {
    signed char tri[256][16];
    unsigned char ntri[256];
};

const Tables& host_tables() {
    static Tables t;
    static std::once_flag once;
    std::call_once(once, [] {
        for (int cs = 0; cs < 256; ++cs) {
            int nxt[12];
            for (int e = 0; e < 12; ++e) nxt[e] = -1;
            for (const auto& quad : kFaces) {
                int enters[2], exits[2], ne = 0, nx = 0;
                for (int k = 0; k < 4; ++k) {
                    const int a = (cs >> quad[k]) & 1, b = (cs >> quad[(k + 1) & 3]) & 1;
                    if (a && !b) exits[nx++] = k;
                    else if (!a && b) enters[ne++] = k;
                }
                for (int i = 0; i < ne; ++i) {
                    // the inside arc entered here ends at the first exit after it (ccw): ambiguous faces isolate inside corners
                    int best = -1, bd = 5;
                    for (int j = 0; j < nx; ++j) {
                        const int dd = (exits[j] - enters[i] + 4) & 3;
                        if (dd < bd) { bd = dd; best = exits[j]; }
                    }
                    nxt[edge_of(quad[enters[i]], quad[(enters[i] + 1) & 3])] = edge_of(quad[best], quad[(best + 1) & 3]);
                }
            }
            bool seen[12] = {};
            int n = 0;
            for (int e = 0; e < 16; ++e) t.tri[cs][e] = -1;
            for (int start = 0; start < 12; ++start) {
                if (nxt[start] < 0 || seen[start]) continue;
                int loop[12], len = 0;
                for (int e = start; !seen[e]; e = nxt[e]) { seen[e] = true; loop[len++] = e; }
                // fan apex: the first rotation with no diagonal lying in a cube face (the neighbouring cube could draw the same
                // diagonal on the shared face: four triangles on one edge)
                int best = 0, best_bad = 1 << 30;
                for (int r = 0; r < len; ++r) {
                    int bad = 0;
                    for (int i = 2; i < len - 1; ++i) bad += share_face(loop[r], loop[(r + i) % len]) ? 1 : 0;
                    if (bad < best_bad) { best_bad = bad; best = r; }
                }
                for (int i = 1; i + 1 < len; ++i) {
                    t.tri[cs][n++] = (signed char)loop[best];
                    t.tri[cs][n++] = (signed char)loop[(best + i) % len];
                    t.tri[cs][n++] = (signed char)loop[(best + i + 1) % len];
                }
            }
            t.ntri[cs] = (unsigned char)(n / 3);
        }
    });
    return t;
}

__constant__ signed char c_tri[256][16];
__constant__ unsigned char c_ntri[256];

// __constant__ memory is per device: the tables go once to every GPU that runs marching cubes, the current one of the calling entry point
int upload_tables() {
    static std::mutex mu;
    static std::vector<char> done;                         // by device ordinal
    int dev = 0;
    OAI_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < (int)done.size() && done[dev]) return OAI_OK;
    const Tables& t = host_tables();
    hipError_t err = hipMemcpyToSymbol(HIP_SYMBOL(c_tri), t.tri, sizeof(t.tri));
    if (err == hipSuccess) err = hipMemcpyToSymbol(HIP_SYMBOL(c_ntri), t.ntri, sizeof(t.ntri));
    if (err != hipSuccess) return oai::set_error(OAI_ERR_HIP, "marching-cubes table upload failed: %s", hipGetErrorString(err));
    if (dev >= (int)done.size()) done.resize(dev + 1, 0);
    done[dev] = 1;
    return OAI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// exclusive scan of int32 (counts per voxel), three levels of 1024-element blocks
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kScanBlock = 1024;          // elements per workgroup (256 threads x 4)

__global__ void __launch_bounds__(256) scan_block_kernel(const int* __restrict__ in, int* __restrict__ out, int* __restrict__ block_sums, long long n) {
    __shared__ int wsum[4];
    const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = base + i < n ? in[base + i] : 0;
    const int tsum = v[0] + v[1] + v[2] + v[3];
    int incl = tsum;                                                   // inclusive scan over the wave (DPP-free: shuffles)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int run = woff + incl - tsum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (block_sums && threadIdx.x == 255) block_sums[blockIdx.x] = woff + incl;
}

__global__ void __launch_bounds__(256) scan_add_kernel(int* __restrict__ out, const int* __restrict__ block_offsets, long long n) {
    const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    const int off = block_offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (base + i < n) out[base + i] += off;
}

size_t scan_scratch_ints(long long n) {          // block sums of every level
    size_t total = 0;
    while (n > kScanBlock) {
        n = (n + kScanBlock - 1) / kScanBlock;
        total += (size_t)((n + 63) / 64 * 64);
    }
    return total + 64;
}

// out[i] = sum in[0..i); returns through *total_dev (device int, may alias scratch tail) nothing -- the caller reads
// in[n-1] + out[n-1].  scratch: scan_scratch_ints(n) ints.
int exclusive_scan(const int* in, int* out, long long n, int* scratch, hipStream_t st) {
    const long long nb = (n + kScanBlock - 1) / kScanBlock;
    if (nb <= 1) {
        scan_block_kernel<<<1, 256, 0, st>>>(in, out, nullptr, n);
        OAI_CHECK_LAUNCH();
        return OAI_OK;
    }
    int* sums = scratch;
    scan_block_kernel<<<(unsigned)nb, 256, 0, st>>>(in, out, sums, n);
    OAI_CHECK_LAUNCH();
    if (int rc = exclusive_scan(sums, sums, nb, scratch + (nb + 63) / 64 * 64, st)) return rc;      // in place
    scan_add_kernel<<<(unsigned)nb, 256, 0, st>>>(out, sums, n);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// marching cubes
// ---------------------------------------------------------------------------------------------------------------------
// per voxel: bits 0..2 = the grid edge from this voxel along +x / +y / +z changes sign; vcount = popcount; tcount = triangles of
// the cell whose lowest corner is this voxel (0 on the last plane / row / column)
__global__ void __launch_bounds__(256) mc_classify_kernel(const float* __restrict__ vol, int D, int H, int W, float iso,
                                                          unsigned char* __restrict__ flags, int* __restrict__ vcount, int* __restrict__ tcount) {
    const long long n = (long long)D * H * W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)W * H));
    const long long sy = W, sz = (long long)W * H;
    const bool in0 = vol[i] > iso;
    const bool hx = x + 1 < W, hy = y + 1 < H, hz = z + 1 < D;
    const bool i1 = hx && vol[i + 1] > iso, i2 = hy && vol[i + sy] > iso, i4 = hz && vol[i + sz] > iso;
    unsigned f = 0;
    if (hx && i1 != in0) f |= 1;
    if (hy && i2 != in0) f |= 2;
    if (hz && i4 != in0) f |= 4;
    flags[i] = (unsigned char)f;
    vcount[i] = __popc(f);
    int nt = 0;
    if (hx && hy && hz) {
        unsigned cs = (in0 ? 1u : 0u) | (i1 ? 2u : 0u) | (i2 ? 4u : 0u) | (i4 ? 16u : 0u);
        cs |= vol[i + sy + 1] > iso ? 8u : 0u;
        cs |= vol[i + sz + 1] > iso ? 32u : 0u;
        cs |= vol[i + sz + sy] > iso ? 64u : 0u;
        cs |= vol[i + sz + sy + 1] > iso ? 128u : 0u;
        nt = c_ntri[cs];
    }
    tcount[i] = nt;
}

__global__ void __launch_bounds__(256) mc_emit_kernel(const float* __restrict__ vol, int D, int H, int W, float iso, float sx, float sy_, float sz_,
                                                      const unsigned char* __restrict__ flags, const int* __restrict__ voff, const int* __restrict__ toff,
                                                      float* __restrict__ verts, int* __restrict__ faces) {
    const long long n = (long long)D * H * W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)W * H));
    const long long sy = W, sz = (long long)W * H;
    const unsigned f = flags[i];
    const float v0 = vol[i];
    // ---- vertices owned by this voxel, in axis order
    if (f) {
        int o = voff[i];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            if (f & (1u << ax)) {
                const float v1 = vol[i + (ax == 0 ? 1 : ax == 1 ? sy : sz)];
                const float t = (iso - v0) / (v1 - v0);
                float p[3] = {(float)x, (float)y, (float)z};
                p[ax] += t;
                verts[3 * (long long)o + 0] = p[0] * sx;
                verts[3 * (long long)o + 1] = p[1] * sy_;
                verts[3 * (long long)o + 2] = p[2] * sz_;
                ++o;
            }
    }
    // ---- triangles of the cell
    if (x + 1 < W && y + 1 < H && z + 1 < D) {
        unsigned cs = v0 > iso ? 1u : 0u;
        cs |= vol[i + 1] > iso ? 2u : 0u;
        cs |= vol[i + sy] > iso ? 4u : 0u;
        cs |= vol[i + sy + 1] > iso ? 8u : 0u;
        cs |= vol[i + sz] > iso ? 16u : 0u;
        cs |= vol[i + sz + 1] > iso ? 32u : 0u;
        cs |= vol[i + sz + sy] > iso ? 64u : 0u;
        cs |= vol[i + sz + sy + 1] > iso ? 128u : 0u;
        const int nt = c_ntri[cs];
        if (nt) {
            const long long t0 = toff[i];
            for (int k = 0; k < 3 * nt; ++k) {
                const int e = c_tri[cs][k];
                const int ax = e >> 2, j = e & 3, a = j & 1, b = j >> 1;
                const int ox = ax == 0 ? 0 : a, oy = ax == 0 ? a : (ax == 1 ? 0 : b), oz = ax == 2 ? 0 : b;
                const long long owner = i + ox + oy * sy + oz * sz;
                const unsigned of = flags[owner];
                faces[3 * t0 + k] = voff[owner] + __popc(of & ((1u << ax) - 1u));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Laplacian smoothing (Jacobi sweep over the CSR edge graph)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) smooth_kernel(const float* __restrict__ in, float* __restrict__ out, long long n,
                                                     const int* __restrict__ off, const int* __restrict__ nbr, float relax) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = off[i], e = off[i + 1];
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    if (e == b) { out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z; return; }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int k = b; k < e; ++k) {
        const long long j = nbr[k];
        sx += in[3 * j]; sy += in[3 * j + 1]; sz += in[3 * j + 2];
    }
    const float d = (float)(e - b);
    out[3 * i] = x + relax * (sx / d - x);
    out[3 * i + 1] = y + relax * (sy / d - y);
    out[3 * i + 2] = z + relax * (sz / d - z);
}

// ---------------------------------------------------------------------------------------------------------------------
// unsigned distance from points to a triangle mesh: one lane per point, triangles streamed through LDS
// ---------------------------------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// squared distance from p to triangle (a, a + ab, a + ac): the Voronoi-region ladder of Ericson, Real-Time Collision Detection 5.1.5,
// for the vertices and edges.  Over the interior it is the distance to the plane, (ap . n)^2 / |n|^2 with n = ab x ac, not
// Ericson's |p - (a + v ab + w ac)|^2: his v and w divide by va + vb + vc -- |n|^2 again, but as a sum of cancelling products of size
// |ap|^2 |ab| |ac| -- so their float32 error grows like 2^-24 |ap|^2 / sin^2 of the triangle's angle and moved the foot point along a
// 1:100 needle by 1e-4 of its length; n loses 2^-24 / sin, once.  Only for well-shaped triangles: see kThin.
__device__ __forceinline__ float tri_dist2(V3 p, V3 a, V3 ab, V3 ac) {
    const V3 ap = p - a;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    V3 q;
    if (d1 <= 0.0f && d2 <= 0.0f) q = a;
    else {
        const V3 bp = ap - ab;
        const float d3 = dot(ab, bp), d4 = dot(ac, bp);
        if (d3 >= 0.0f && d4 <= d3) q = a + ab;
        else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) q = a + ab * (d1 / (d1 - d3));
            else {
                const V3 cp = ap - ac;
                const float d5 = dot(ab, cp), d6 = dot(ac, cp);
                if (d6 >= 0.0f && d5 <= d6) q = a + ac;
                else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) q = a + ac * (d2 / (d2 - d6));
                    else {
                        const float va = d3 * d6 - d5 * d4;
                        if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
                            const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                            q = a + ab + (ac - ab) * w;
                        } else {
                            const V3 n = cross(ab, ac);
                            const float s = dot(ap, n);
                            return s * s * __builtin_amdgcn_rcpf(dot(n, n));        // v_rcp_f32: 1 ulp on a squared distance
                        }
                    }
                }
            }
        }
    }
    const V3 d = p - q;
    return dot(d, d);
}

// The ladder is float32 and assumes a triangle.  With a == b its edge parameter is 0/0 (fminf drops the NaN, and the triangle with it);
// on a needle the signs of va, vb, vc that pick the region are noise.  A triangle with |ab x ac|^2 <= kThin |ab|^2 |ac|^2 -- the sine of
// the angle at a at most 1e-2, zero area included -- takes tri_dist2_thin instead.  The test is made once per triangle, outside the hot
// loops (by the lane that stages it for the brute-force kernel, by grid_bin_kernel for the grid), with every rounding spelled out so
// that the two kernels class a borderline triangle alike.
constexpr float kThin = 1e-4f;
__device__ __forceinline__ float dot_rn(V3 a, V3 b) { return __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmul_rn(a.x, b.x))); }
__device__ __forceinline__ bool is_thin(V3 ab, V3 ac) {
    const V3 n = {__fmaf_rn(ab.y, ac.z, -__fmul_rn(ab.z, ac.y)), __fmaf_rn(ab.z, ac.x, -__fmul_rn(ab.x, ac.z)), __fmaf_rn(ab.x, ac.y, -__fmul_rn(ab.y, ac.x))};
    return dot_rn(n, n) <= __fmul_rn(kThin, __fmul_rn(dot_rn(ab, ab), dot_rn(ac, ac)));
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// squared distance from a point at `up` (relative to the segment's start) to the segment of direction e; no length: its start
__device__ __forceinline__ double seg_dist2(D3 up, D3 e) {
    const double ee = dot(e, e);
    const double t = ee > 0.0 ? fmin(fmax(dot(up, e) / ee, 0.0), 1.0) : 0.0;
    const D3 d = {up.x - t * e.x, up.y - t * e.y, up.z - t * e.z};
    return dot(d, d);
}

// The same squared distance without the ladder, in double: the nearest of the three edges, and the plane distance where the triangle
// has a normal and the point projects inside it (three same-side tests against n = ab x ac).  No division can be 0/0, so no triangle
// yields NaN; a triangle without area is exactly its edges.  Rare, hence out of line.
__device__ __noinline__ float tri_dist2_thin(V3 p, V3 a, V3 ab, V3 ac) {
    const D3 AB = {ab.x, ab.y, ab.z}, AC = {ac.x, ac.y, ac.z};
    const D3 ap = D3{p.x, p.y, p.z} - D3{a.x, a.y, a.z}, bp = ap - AB, cp = ap - AC, BC = AC - AB;
    double best = fmin(fmin(seg_dist2(ap, AB), seg_dist2(ap, AC)), seg_dist2(bp, BC));
    const D3 n = cross(AB, AC);
    const double nn = dot(n, n);
    if (nn > 0.0 && dot(cross(AB, ap), n) >= 0.0 && dot(cross(BC, bp), n) >= 0.0 && dot(cross(cp, AC), n) >= 0.0) {   // ca x cp = cp x ac
        const double s = dot(ap, n);
        best = fmin(best, s * s / nn);
    }
    return (float)best;
}

constexpr int kTriTile = 512;

__global__ void __launch_bounds__(256) point_distance_kernel(const float* __restrict__ pts, long long np, const float* __restrict__ verts,
                                                             const int* __restrict__ faces, long long nt, float* __restrict__ dist) {
    __shared__ float tri[kTriTile][9];          // a, ab, ac
    __shared__ float thin_edges[kTriTile][6];   // ab, ac of the tile's thin triangles, in the order they were claimed
    __shared__ int thin_list[kTriTile];         // their positions in the tile
    __shared__ int n_thin;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < np;
    const V3 p = live ? V3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]} : V3{0.f, 0.f, 0.f};
    float best = 3.4e38f;
    for (long long t0 = 0; t0 < nt; t0 += kTriTile) {
        const int cnt = (int)(nt - t0 < kTriTile ? nt - t0 : kTriTile);
        __syncthreads();
        if (threadIdx.x == 0) n_thin = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += 256) {
            const int* f = faces + 3 * (t0 + k);
            const float* a = verts + 3 * (long long)f[0];
            const float* b = verts + 3 * (long long)f[1];
            const float* c = verts + 3 * (long long)f[2];
            V3 ab = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            if (is_thin(ab, ac)) {
                // out of the hot loop, which then sees the one-point triangle (a, a, a): its distance, |p - a|, is no less than the
                // real triangle's, so the minimum is unharmed, and the loop needs no branch
                const int slot = atomicAdd(&n_thin, 1);
                thin_list[slot] = k;
                thin_edges[slot][0] = ab.x; thin_edges[slot][1] = ab.y; thin_edges[slot][2] = ab.z;
                thin_edges[slot][3] = ac.x; thin_edges[slot][4] = ac.y; thin_edges[slot][5] = ac.z;
                ab = ac = V3{0.f, 0.f, 0.f};
            }
            tri[k][0] = a[0]; tri[k][1] = a[1]; tri[k][2] = a[2];
            tri[k][3] = ab.x; tri[k][4] = ab.y; tri[k][5] = ab.z;
            tri[k][6] = ac.x; tri[k][7] = ac.y; tri[k][8] = ac.z;
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k)          // LDS broadcast reads: every lane wants the same triangle
                best = fminf(best, tri_dist2(p, V3{tri[k][0], tri[k][1], tri[k][2]}, V3{tri[k][3], tri[k][4], tri[k][5]}, V3{tri[k][6], tri[k][7], tri[k][8]}));
            for (int j = 0; j < n_thin; ++j) {     // (min is exact, so the order the slots were claimed in does not show)
                const int k = thin_list[j];
                best = fminf(best, tri_dist2_thin(p, V3{tri[k][0], tri[k][1], tri[k][2]}, V3{thin_edges[j][0], thin_edges[j][1], thin_edges[j][2]},
                                                  V3{thin_edges[j][3], thin_edges[j][4], thin_edges[j][5]}));
            }
        }
    }
    if (live) dist[i] = sqrtf(best);
}


// ---------------------------------------------------------------------------------------------------------------------
// the same distance with a uniform-grid broad phase: triangles are binned into the cells their bounding boxes overlap
// (count -> prefix sum -> fill), a point walks the cells around it ring by ring and stops when the best distance found is
// within the radius already covered, less a slack for the cell arithmetic (kRingSlack).  Same closest-point routine as the
// brute-force kernel, and every triangle that could be the nearest is visited: the two agree up to the rounding of their own
// (separately inlined) arithmetic, provided every triangle lies inside the grid box the caller describes.
// ---------------------------------------------------------------------------------------------------------------------
constexpr float kRingSlack = 1.0f / 1024.0f;       // cells

using oai::UniformGrid;

template <bool FILL>
__global__ void __launch_bounds__(256) grid_bin_kernel(const float* __restrict__ verts, const int* __restrict__ faces, long long nt, UniformGrid g,
                                                       int* __restrict__ cell_count /*FILL: running fill cursor*/, const int* __restrict__ cell_start,
                                                       int* __restrict__ tri_list) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const float* va = verts + 3 * (long long)faces[3 * t];
    const float* vb = verts + 3 * (long long)faces[3 * t + 1];
    const float* vc = verts + 3 * (long long)faces[3 * t + 2];
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = va[k], b = vb[k], c = vc[k];
        lo[k] = oai::grid_cell(g, k, fminf(a, fminf(b, c)));
        hi[k] = oai::grid_cell(g, k, fmaxf(a, fmaxf(b, c)));
    }
    // a thin triangle (is_thin) is listed as ~t, which is negative: the walk sets it aside for tri_dist2_thin without looking at it
    int entry = (int)t;
    if (FILL && is_thin(V3{vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]}, V3{vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]})) entry = ~entry;
    oai::grid_walk_box(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], [&](int x, int y, int z) {
        const int cell = oai::grid_index(g, x, y, z);
        const int slot = atomicAdd(&cell_count[cell], 1);
        if (FILL) tri_list[cell_start[cell] + slot] = entry;
    });
}

__global__ void __launch_bounds__(256) grid_distance_kernel(const float* __restrict__ pts, long long np, const float* __restrict__ verts,
                                                            const int* __restrict__ faces, UniformGrid g, const int* __restrict__ cell_start,
                                                            const int* __restrict__ tri_list, float* __restrict__ dist) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const V3 p = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const int cx = oai::grid_cell(g, 0, p.x), cy = oai::grid_cell(g, 1, p.y), cz = oai::grid_cell(g, 2, p.z);
    const int rmax = oai::grid_rmax(g, cx, cy, cz);
    const float h = (float)g.h;                     // exact: the entry point's cell size is a float
    float best = 3.4e38f;
    // Lanes of a wave visit different triangles, so a thin one (a negative list entry) handled where it is met would make the whole
    // wave step through the double path each time any lane meets one.  It waits in `pending` instead -- until the lane meets the next,
    // or the ring ends -- which leaves the wave a few such steps per point rather than one per visited cell.  `best` is complete again
    // before each stop test.
    int pending = -1;
    auto flush = [&]() {
        if (pending < 0) return;
        const int* f = faces + 3 * (long long)pending;
        const float* a = verts + 3 * (long long)f[0];
        const float* b = verts + 3 * (long long)f[1];
        const float* c = verts + 3 * (long long)f[2];
        const V3 A = {a[0], a[1], a[2]};
        best = fminf(best, tri_dist2_thin(p, A, V3{b[0], b[1], b[2]} - A, V3{c[0], c[1], c[2]} - A));
        pending = -1;
    };
    for (int r = 0; r <= rmax; ++r) {
        flush();
        // triangles not visited after ring r-1 lie in cells at Chebyshev distance >= r from the point's cell, AS grid_cell COMPUTES
        // both: in float64 with a rounded 1 / h, which can put a coordinate next to a cell boundary into the neighbouring cell.  The
        // slip is below 3 * 2^-52 * 512 = 3.5e-13 cells per coordinate (the subtraction, 1 / h and the product each round once, on at
        // most 512 cells), so such a triangle is at least (r - 1 - 2 * 3.5e-13) * h from the point's projection onto the grid box,
        // hence from the point; kRingSlack = 2^-10 cells covers both slips, and the float32 rounding of `covered`, with room to spare
        const float covered = fmaxf((float)(r - 1) - kRingSlack, 0.0f) * h;
        if (r > 0 && best <= covered * covered) break;
        oai::grid_walk_shell(g, cx, cy, cz, r, [&](int x, int y, int z) {
            const int cell = oai::grid_index(g, x, y, z);
            for (int k = cell_start[cell]; k < cell_start[cell + 1]; ++k) {
                const int t = tri_list[k];
                if (t < 0) { flush(); pending = ~t; continue; }
                const int* f = faces + 3 * (long long)t;
                const float* a = verts + 3 * (long long)f[0];
                const float* b = verts + 3 * (long long)f[1];
                const float* c = verts + 3 * (long long)f[2];
                const V3 A = {a[0], a[1], a[2]};
                best = fminf(best, tri_dist2(p, A, V3{b[0], b[1], b[2]} - A, V3{c[0], c[1], c[2]} - A));
            }
        });
    }
    flush();
    dist[i] = sqrtf(best);
}

// Workspaces: one struct of typed pointers per entry-point family, filled by one carve() that returns the bytes walked (oai::Ws,
// common.h): over a null base that is the *_workspace_bytes answer, over the caller's buffer the carving.
struct GridWs { int *count, *start, *list, *scratch; };
size_t carve(GridWs& w, const void* base, long long ncells, long long nt) {
    oai::Ws ws(base);
    w.count = ws.take<int>(ncells + 1);
    w.start = ws.take<int>(ncells + 1);
    w.list = ws.take<int>(nt * 8);
    w.scratch = ws.take<int>(scan_scratch_ints(ncells + 1));
    return ws.off;
}

struct McWs { unsigned char* flags; int *vcount, *tcount, *voff, *toff, *scratch; };
size_t carve(McWs& w, const void* base, long long n) {
    oai::Ws ws(base);
    w.flags = ws.take<unsigned char>(n);
    w.vcount = ws.take<int>(n);
    w.tcount = ws.take<int>(n);
    w.voff = ws.take<int>(n);
    w.toff = ws.take<int>(n);
    w.scratch = ws.take<int>(scan_scratch_ints(n));
    return ws.off;
}

}  // namespace

namespace oai {     // the scan and the bucket lists built on it, for every source of the library (common.h)
size_t scan_scratch_bytes(long long n) { return scan_scratch_ints(n) * 4; }
int exclusive_scan_i32(const int* in, int* out, long long n, int* scratch, hipStream_t st) { return exclusive_scan(in, out, n, scratch, st); }

int bucket_clear(int* count, long long n, hipStream_t st) {
    OAI_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)(n + 1) * 4, st));
    return OAI_OK;
}
int bucket_starts(int* count, int* start, long long n, int* scratch, hipStream_t st) {
    if (int rc = exclusive_scan(count, start, n + 1, scratch, st)) return rc;
    return bucket_clear(count, n, st);
}
}  // namespace oai

extern "C" {

int oai_mc_table(signed char* out_256x16) {
    OAI_CHECK_ARG(out_256x16, "oai_mc_table: null pointer");
    std::memcpy(out_256x16, host_tables().tri, sizeof(host_tables().tri));
    return OAI_OK;
}

size_t oai_mc_workspace_bytes(int D, int H, int W) {
    if (D < 2 || H < 2 || W < 2) return 0;
    McWs w;
    return carve(w, nullptr, (long long)D * H * W);
}

int oai_mc_count(const float* vol_dev, int D, int H, int W, float iso, void* ws_dev, size_t ws_bytes,
                 long long* n_verts, long long* n_tris, void* stream) {
    OAI_CHECK_ARG(vol_dev && ws_dev && n_verts && n_tris, "oai_mc_count: null pointer");
    OAI_CHECK_ARG(D >= 2 && H >= 2 && W >= 2, "oai_mc_count: every axis needs at least 2 voxels");
    const long long n = (long long)D * H * W;
    OAI_CHECK_ARG(n < (1LL << 31) / 3, "oai_mc_count: volume too large for 32-bit vertex ids");
    McWs w;
    OAI_CHECK_WORKSPACE("oai_mc_count", ws_bytes, carve(w, ws_dev, n));
    if (int rc = upload_tables()) return rc;
    hipStream_t st = (hipStream_t)stream;
    mc_classify_kernel<<<oai::cdiv(n, 256), 256, 0, st>>>(vol_dev, D, H, W, iso, w.flags, w.vcount, w.tcount);
    OAI_CHECK_LAUNCH();
    if (int rc = exclusive_scan(w.vcount, w.voff, n, w.scratch, st)) return rc;
    if (int rc = exclusive_scan(w.tcount, w.toff, n, w.scratch, st)) return rc;
    int last[4];                                                // the caller sizes its output arrays from the counts
    if (int rc = oai::read_ints(last, {w.vcount + n - 1, w.voff + n - 1, w.tcount + n - 1, w.toff + n - 1}, st)) return rc;
    *n_verts = (long long)last[0] + last[1];
    *n_tris = (long long)last[2] + last[3];
    return OAI_OK;
}

int oai_mc_emit(const float* vol_dev, int D, int H, int W, float iso, const float spacing_xyz[3], const void* ws_dev,
                float* verts_dev, int* faces_dev, void* stream) {
    OAI_CHECK_ARG(vol_dev && ws_dev && spacing_xyz, "oai_mc_emit: null pointer");
    OAI_CHECK_ARG(D >= 2 && H >= 2 && W >= 2, "oai_mc_emit: every axis needs at least 2 voxels");
    const long long n = (long long)D * H * W;
    McWs w;                                                     // read only: the kernel takes these pointers as const
    carve(w, ws_dev, n);
    mc_emit_kernel<<<oai::cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(vol_dev, D, H, W, iso, spacing_xyz[0], spacing_xyz[1], spacing_xyz[2],
                                                                        w.flags, w.voff, w.toff, verts_dev, faces_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_mesh_smooth(const float* verts_in_dev, long long n_verts, const int* offsets_dev, const int* nbrs_dev, int iterations,
                    float relaxation, float* tmp_dev, float* verts_out_dev, void* stream) {
    OAI_CHECK_ARG(verts_in_dev && offsets_dev && nbrs_dev && tmp_dev && verts_out_dev, "oai_mesh_smooth: null pointer");
    OAI_CHECK_ARG(n_verts >= 0 && iterations >= 0, "oai_mesh_smooth: negative size");
    hipStream_t st = (hipStream_t)stream;
    if (n_verts == 0) return OAI_OK;
    if (iterations == 0) {
        OAI_CHECK_HIP(hipMemcpyAsync(verts_out_dev, verts_in_dev, (size_t)n_verts * 12, hipMemcpyDeviceToDevice, st));
        return OAI_OK;
    }
    // ping-pong so that the last sweep lands in verts_out
    const float* src = verts_in_dev;
    for (int it = 0; it < iterations; ++it) {
        float* dst = ((iterations - it) & 1) ? verts_out_dev : tmp_dev;
        smooth_kernel<<<oai::cdiv(n_verts, 256), 256, 0, st>>>(src, dst, n_verts, offsets_dev, nbrs_dev, relaxation);
        OAI_CHECK_LAUNCH();
        src = dst;
    }
    return OAI_OK;
}

int oai_mesh_point_distance(const float* points_dev, long long n_points, const float* verts_dev, const int* faces_dev,
                            long long n_tris, float* dist_dev, void* stream) {
    OAI_CHECK_ARG(n_points >= 0 && n_tris > 0, "oai_mesh_point_distance: needs at least one triangle");
    OAI_CHECK_ARG(verts_dev && faces_dev && ((points_dev && dist_dev) || n_points == 0), "oai_mesh_point_distance: null pointer");
    if (n_points == 0) return OAI_OK;
    point_distance_kernel<<<oai::cdiv(n_points, 256), 256, 0, (hipStream_t)stream>>>(points_dev, n_points, verts_dev, faces_dev, n_tris, dist_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_mesh_grid_workspace_bytes(const int grid_dims_xyz[3], long long n_tris) {
    if (!grid_dims_xyz || n_tris <= 0) return 0;
    GridWs w;
    return carve(w, nullptr, (long long)grid_dims_xyz[0] * grid_dims_xyz[1] * grid_dims_xyz[2], n_tris);
}

int oai_mesh_point_distance_grid(const float* points_dev, long long n_points, const float* verts_dev, const int* faces_dev, long long n_tris,
                                 const float grid_lo_xyz[3], float cell_size, const int grid_dims_xyz[3],
                                 void* workspace_dev, size_t workspace_bytes, float* dist_dev, void* stream) {
    OAI_CHECK_ARG(n_points >= 0 && n_tris > 0 && cell_size > 0.0f, "oai_mesh_point_distance_grid: needs triangles and a positive cell size");
    OAI_CHECK_ARG(verts_dev && faces_dev && grid_lo_xyz && grid_dims_xyz && workspace_dev && ((points_dev && dist_dev) || n_points == 0),
                  "oai_mesh_point_distance_grid: null pointer");
    OAI_CHECK_ARG(grid_dims_xyz[0] > 0 && grid_dims_xyz[1] > 0 && grid_dims_xyz[2] > 0, "oai_mesh_point_distance_grid: empty grid");
    const long long ncells = (long long)grid_dims_xyz[0] * grid_dims_xyz[1] * grid_dims_xyz[2];
    OAI_CHECK_ARG(ncells < (1LL << 30), "oai_mesh_point_distance_grid: grid too fine");
    GridWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_point_distance_grid", workspace_bytes, carve(w, workspace_dev, ncells, n_tris));
    if (n_points == 0) return OAI_OK;
    hipStream_t st = (hipStream_t)stream;
    const double lo[3] = {grid_lo_xyz[0], grid_lo_xyz[1], grid_lo_xyz[2]};          // widened exactly: the ABI stays float
    const UniformGrid g = oai::make_uniform_grid(lo, (double)cell_size, grid_dims_xyz);
    if (int rc = oai::bucket_clear(w.count, ncells, st)) return rc;
    grid_bin_kernel<false><<<oai::cdiv(n_tris, 256), 256, 0, st>>>(verts_dev, faces_dev, n_tris, g, w.count, nullptr, nullptr);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::bucket_starts(w.count, w.start, ncells, w.scratch, st)) return rc;
    int total = 0;
    if (int rc = oai::read_ints(&total, {w.start + ncells}, st)) return rc;
    if ((long long)total > n_tris * 8)          // a triangle longer than a cell overlaps more than 8 cells: the caller's cell size is too small
        return oai::set_error(OAI_ERR_ARG, "oai_mesh_point_distance_grid: %d triangle-cell pairs > 8 per triangle; cell_size %g must be >= the longest edge",
                              total, (double)cell_size);
    grid_bin_kernel<true><<<oai::cdiv(n_tris, 256), 256, 0, st>>>(verts_dev, faces_dev, n_tris, g, w.count, w.start, w.list);
    OAI_CHECK_LAUNCH();
    grid_distance_kernel<<<oai::cdiv(n_points, 256), 256, 0, st>>>(points_dev, n_points, verts_dev, faces_dev, g, w.start, w.list, dist_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
