// Thickness image for gfx950: the atlas' 2-D projection rasterised once, every knee's thickness gathered through it.
//
// map_attributes puts every knee's thickness on the ATLAS inner mesh, so all knees share one 2-D projection (project_thickness of the
// atlas mesh).  FullDemo.ipynb draws that projection as a scatter plot; a cohort comparison wants an image on a fixed grid (the same
// pixel = the same atlas location).  That costs one rasterisation per atlas and one gather per knee:
//   oai_thickness_image_build   per pixel: the face of the projected atlas mesh that owns the pixel centre, its three point indices
//                               and the barycentric weights of the centre
//   oai_thickness_image_apply   per pixel and knee: w0 t[a] + w1 t[b] + w2 t[c]
//
// Every decision (covered or not, which face owns) is fp64 with contraction off, written so that a numpy restatement performs the same
// operations in the same order (tests/thickness_image_ref.py).  The owner of a pixel is the SMALLEST covering face index, taken with an
// integer atomicMin: independent of the order in which faces arrive, the same bits on every run.  No float atomics, no MFMA: build is a
// once-per-atlas scan of small boxes, apply is a pure gather.
#include "common.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;                       // threads per block
constexpr int kWave = 64;                     // one wave scans one face's box
constexpr int kFacesPerBlock = kT / kWave;
constexpr size_t kHead = 256;                 // workspace: the covered-pixel counter, then one box per face

struct Raster {
    double lo_u, lo_v, step_u, step_v;
    int height, width;
};

struct Box { int i0, i1, j0, j1; };           // pixel columns [i0, i1] x rows [j0, j1]; i1 < i0 = the face covers nothing

__device__ __forceinline__ double centre_u(const Raster& r, int i) { return r.lo_u + ((double)i + 0.5) * r.step_u; }
__device__ __forceinline__ double centre_v(const Raster& r, int j) { return r.lo_v + ((double)j + 0.5) * r.step_v; }

struct Tri {
    double au, av, bu, bv, cu, cv;
    bool flip;                                // area < 0: the edge functions are negated
};

// the three edge functions of the pixel centre (pu, pv): e0 on B->C (the weight of A), e1 on C->A, e2 on A->B
__device__ __forceinline__ void edges(const Tri& t, double pu, double pv, double& e0, double& e1, double& e2) {
    e0 = (t.cu - t.bu) * (pv - t.bv) - (t.cv - t.bv) * (pu - t.bu);
    e1 = (t.au - t.cu) * (pv - t.cv) - (t.av - t.cv) * (pu - t.cu);
    e2 = (t.bu - t.au) * (pv - t.av) - (t.bv - t.av) * (pu - t.au);
    if (t.flip) { e0 = -e0; e1 = -e1; e2 = -e2; }
}

// false = the face is skipped (marked, an index outside the points, a coordinate that is not finite, zero area)
__device__ __forceinline__ bool load_tri(const double* __restrict__ uv, long long n_pts, const int* __restrict__ faces,
                                         const unsigned char* __restrict__ skip, long long f, Tri& t) {
    if (skip && skip[f]) return false;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || a >= n_pts || b >= n_pts || c >= n_pts) return false;
    t.au = uv[2 * (long long)a]; t.av = uv[2 * (long long)a + 1];
    t.bu = uv[2 * (long long)b]; t.bv = uv[2 * (long long)b + 1];
    t.cu = uv[2 * (long long)c]; t.cv = uv[2 * (long long)c + 1];
    if (!(isfinite(t.au) && isfinite(t.av) && isfinite(t.bu) && isfinite(t.bv) && isfinite(t.cu) && isfinite(t.cv))) return false;
    const double area = (t.bu - t.au) * (t.cv - t.av) - (t.bv - t.av) * (t.cu - t.au);
    if (!(area != 0.0) || !isfinite(area)) return false;
    t.flip = area < 0.0;
    return true;
}

// first / last pixel whose centre can lie in [x0, x1], one pixel of margin on either side against rounding, clamped to the image
__device__ __forceinline__ void pixel_span(double x0, double x1, double lo, double step, int n, int& p0, int& p1) {
    double a = floor((x0 - lo) / step - 0.5) - 1.0, b = ceil((x1 - lo) / step - 0.5) + 1.0;
    a = a >= 0.0 ? a : 0.0;                    // (the coordinates are finite and step > 0: no NaN here)
    b = b <= (double)(n - 1) ? b : (double)(n - 1);
    if (a > (double)(n - 1) || b < 0.0) { p0 = 0; p1 = -1; return; }
    p0 = (int)a; p1 = (int)b;
}

__global__ void __launch_bounds__(kT) face_box_kernel(const double* __restrict__ uv, long long n_pts, const int* __restrict__ faces,
                                                      long long n_faces, const unsigned char* __restrict__ skip, Raster r,
                                                      Box* __restrict__ box) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    if (f >= n_faces) return;
    Tri t;
    Box b{0, -1, 0, -1};
    if (load_tri(uv, n_pts, faces, skip, f, t)) {
        pixel_span(fmin(t.au, fmin(t.bu, t.cu)), fmax(t.au, fmax(t.bu, t.cu)), r.lo_u, r.step_u, r.width, b.i0, b.i1);
        pixel_span(fmin(t.av, fmin(t.bv, t.cv)), fmax(t.av, fmax(t.bv, t.cv)), r.lo_v, r.step_v, r.height, b.j0, b.j1);
        if (b.j1 < b.j0) { b.i0 = 0; b.i1 = -1; }
    }
    box[f] = b;
}

__global__ void __launch_bounds__(kT) fill_owner_kernel(int* __restrict__ owner, long long n) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p < n) owner[p] = INT_MAX;
}

// one wave per face: its lanes walk the face's box, a covered pixel takes min(owner, f)
__global__ void __launch_bounds__(kT) cover_kernel(const double* __restrict__ uv, long long n_pts, const int* __restrict__ faces,
                                                   long long n_faces, const unsigned char* __restrict__ skip, Raster r,
                                                   const Box* __restrict__ box, int* __restrict__ owner) {
    const long long f = (long long)blockIdx.x * kFacesPerBlock + threadIdx.x / kWave;
    if (f >= n_faces) return;
    const Box b = box[f];
    if (b.i1 < b.i0) return;
    Tri t;
    if (!load_tri(uv, n_pts, faces, skip, f, t)) return;
    const int bw = b.i1 - b.i0 + 1;
    const long long n_px = (long long)bw * (b.j1 - b.j0 + 1);
    for (long long k = threadIdx.x % kWave; k < n_px; k += kWave) {
        const int j = b.j0 + (int)(k / bw), i = b.i0 + (int)(k % bw);        // inside [0, height) x [0, width): pixel_span clamps
        double e0, e1, e2;
        edges(t, centre_u(r, i), centre_v(r, j), e0, e1, e2);
        if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) atomicMin(&owner[(long long)j * r.width + i], (int)f);
    }
}

// one thread per pixel: the owner's corners and weights; pixels nobody covers get owner -1, corners 0, weights 0
__global__ void __launch_bounds__(kT) resolve_kernel(const double* __restrict__ uv, long long n_pts, const int* __restrict__ faces,
                                                     Raster r, int* __restrict__ owner, int* __restrict__ corners,
                                                     double* __restrict__ weights, unsigned long long* __restrict__ n_covered) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    const long long n = (long long)r.height * r.width;
    bool covered = false;
    if (p < n) {
        const int f = owner[p];
        int c[3] = {0, 0, 0};
        double w[3] = {0.0, 0.0, 0.0};
        Tri t;
        if (f != INT_MAX && load_tri(uv, n_pts, faces, nullptr, f, t)) {
            covered = true;
            double e0, e1, e2;
            edges(t, centre_u(r, (int)(p % r.width)), centre_v(r, (int)(p / r.width)), e0, e1, e2);
            const double s = (e0 + e1) + e2;
            w[0] = e0 / s; w[1] = e1 / s; w[2] = e2 / s;
            c[0] = faces[3 * (long long)f]; c[1] = faces[3 * (long long)f + 1]; c[2] = faces[3 * (long long)f + 2];
        } else {
            owner[p] = -1;
        }
        for (int k = 0; k < 3; ++k) { corners[3 * p + k] = c[k]; weights[3 * p + k] = w[k]; }
    }
    const unsigned long long m = __ballot(covered);
    if (threadIdx.x % kWave == 0 && m) atomicAdd(n_covered, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(kT) apply_kernel(const int* __restrict__ owner, const int* __restrict__ corners,
                                                   const double* __restrict__ weights, long long n_px, const float* __restrict__ values,
                                                   long long n_pts, float* __restrict__ image) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p >= n_px) return;
    const float* t = values + (long long)blockIdx.y * n_pts;
    float out = __int_as_float(0x7fc00000);
    if (owner[p] >= 0) {
        const int a = corners[3 * p], b = corners[3 * p + 1], c = corners[3 * p + 2];
        if (a >= 0 && b >= 0 && c >= 0 && a < n_pts && b < n_pts && c < n_pts)      // (a raster built for another mesh must not read outside)
            out = (float)((weights[3 * p] * (double)t[a] + weights[3 * p + 1] * (double)t[b]) + weights[3 * p + 2] * (double)t[c]);
    }
    image[(long long)blockIdx.y * n_px + p] = out;
}

size_t build_bytes(long long n_faces) { return kHead + (size_t)n_faces * sizeof(Box); }

}  // namespace

extern "C" {

size_t oai_thickness_image_workspace_bytes(long long n_faces, int height, int width) {
    if (n_faces <= 0 || height < 1 || width < 1) return 0;
    return build_bytes(n_faces);
}

int oai_thickness_image_build(const double* uv_dev, long long n_pts, const int* faces_dev, long long n_faces, const unsigned char* face_skip_dev,
                              const double lo_host[2], const double step_host[2], int height, int width, void* workspace_dev,
                              size_t workspace_bytes, int* owner_dev, int* corners_dev, double* weights_dev, long long* n_covered_host,
                              void* stream) {
    OAI_CHECK_ARG(uv_dev && faces_dev && lo_host && step_host && workspace_dev && owner_dev && corners_dev && weights_dev && n_covered_host,
                  "oai_thickness_image_build: null pointer");
    OAI_CHECK_ARG(height >= 1 && width >= 1 && (long long)height * width < (1LL << 30), "oai_thickness_image_build: image %d x %d must be 1 .. 2^30-1 pixels",
                  height, width);
    OAI_CHECK_ARG(n_pts > 0 && n_pts < (1LL << 31) && n_faces > 0 && n_faces < (1LL << 31),
                  "oai_thickness_image_build: needs 1 .. 2^31-1 points and faces (got %lld, %lld)", n_pts, n_faces);
    OAI_CHECK_ARG(std::isfinite(lo_host[0]) && std::isfinite(lo_host[1]), "oai_thickness_image_build: the grid origin is not finite");
    OAI_CHECK_ARG(step_host[0] > 0.0 && step_host[1] > 0.0 && std::isfinite(step_host[0]) && std::isfinite(step_host[1]),
                  "oai_thickness_image_build: step (%g, %g) must be finite and > 0", step_host[0], step_host[1]);
    OAI_CHECK_WORKSPACE("oai_thickness_image_build", workspace_bytes, build_bytes(n_faces));
    hipStream_t st = (hipStream_t)stream;
    const Raster r{lo_host[0], lo_host[1], step_host[0], step_host[1], height, width};
    const long long n_px = (long long)height * width;
    unsigned long long* counter = (unsigned long long*)workspace_dev;
    Box* box = (Box*)((char*)workspace_dev + kHead);
    OAI_CHECK_HIP(hipMemsetAsync(counter, 0, sizeof(*counter), st));
    fill_owner_kernel<<<oai::cdiv(n_px, kT), kT, 0, st>>>(owner_dev, n_px);
    OAI_CHECK_LAUNCH();
    face_box_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(uv_dev, n_pts, faces_dev, n_faces, face_skip_dev, r, box);
    OAI_CHECK_LAUNCH();
    cover_kernel<<<oai::cdiv(n_faces, kFacesPerBlock), kT, 0, st>>>(uv_dev, n_pts, faces_dev, n_faces, face_skip_dev, r, box, owner_dev);
    OAI_CHECK_LAUNCH();
    resolve_kernel<<<oai::cdiv(n_px, kT), kT, 0, st>>>(uv_dev, n_pts, faces_dev, r, owner_dev, corners_dev, weights_dev, counter);
    OAI_CHECK_LAUNCH();
    unsigned long long covered = 0;
    OAI_CHECK_HIP(hipMemcpyAsync(&covered, counter, sizeof(covered), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    *n_covered_host = (long long)covered;
    return OAI_OK;
}

int oai_thickness_image_apply(const int* owner_dev, const int* corners_dev, const double* weights_dev, int height, int width,
                              const float* values_dev, long long n_pts, int n_knees, float* image_dev, void* stream) {
    OAI_CHECK_ARG(owner_dev && corners_dev && weights_dev && values_dev && image_dev, "oai_thickness_image_apply: null pointer");
    OAI_CHECK_ARG(height >= 1 && width >= 1 && (long long)height * width < (1LL << 30), "oai_thickness_image_apply: image %d x %d must be 1 .. 2^30-1 pixels",
                  height, width);
    OAI_CHECK_ARG(n_pts > 0 && n_pts < (1LL << 31), "oai_thickness_image_apply: needs 1 .. 2^31-1 points (got %lld)", n_pts);
    OAI_CHECK_ARG(n_knees >= 0 && n_knees <= 65535, "oai_thickness_image_apply: 0 .. 65535 knees per call (got %d)", n_knees);
    if (n_knees == 0) return OAI_OK;
    const long long n_px = (long long)height * width;
    apply_kernel<<<dim3(oai::cdiv(n_px, kT), (unsigned)n_knees), kT, 0, (hipStream_t)stream>>>(owner_dev, corners_dev, weights_dev, n_px, values_dev,
                                                                                               n_pts, image_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
