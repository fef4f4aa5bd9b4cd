// Mesh points pushed through the registration's dense map phi for gfx950: the point form of the resample (csrc/warp.hip).
//
// VolumeResult.phi maps atlas points to patient points (DisplacementTransform: B-physical -> A-physical).  The resample pulls a patient
// image onto the atlas grid through it, voxel by voxel; this pushes single points -- the vertices of a mesh extracted on the atlas grid --
// the same way: affine into network index space, + the trilinearly interpolated displacement when the point lies inside the field's
// buffer (identity outside: ITK's DisplacementFieldTransform), affine out.  It is what itk.transform_mesh_filter does with the
// registration's CompositeTransform; restated from ITK's documented behaviour and unpinned, like the resample (oracle/resample.py).
//   oai_transform_points_through_phi   one thread per point, grid-stride
//
// The displacement at the 8 clamped corners is rebuilt from phi's fp32 planes by the function that phi_to_disp_kernel and
// resample_maps_kernel call (itk_disp, csrc/phi_field.h), so at a lattice point it is the value oai_phi_to_itk_displacement stores.
// Coordinates, the lerp (x, then y, then z) and both affines are fp64 with contraction off, written so that a numpy restatement performs
// the same operations in the same order (tests/mesh_transform_ref.py); the only rounding left open is the final one to float32.  A mesh has
// 10^4 .. 10^5 points: the launch is latency-bound, 24 scattered 4-byte loads per point out of a field that sits in L2 / Infinity Cache
// after the resample.  No LDS, no atomics.
#include "common.h"

#pragma clang fp contract(off)

#include "phi_field.h"      // after the pragma: compiled with contraction off here (see its leading comment)

namespace {

using namespace oai;

constexpr int kT = 256;                       // threads per block

__global__ void __launch_bounds__(kT)
transform_points_kernel(const float* __restrict__ pts, long long n, const float* __restrict__ phi, int Dn, int Hn, int Wn, oai_affine p2n,
                        oai_affine n2o, float* __restrict__ out, unsigned char* __restrict__ inside_out) {
    const long long plane = (long long)Dn * Hn * Wn;
    const double inz = 1.0 / (Dn - 1), iny = 1.0 / (Hn - 1), inx = 1.0 / (Wn - 1);
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        double x, y, z;
        apply(p2n, (double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], x, y, z);
        const bool inside = inside_buffer(x, y, z, Wn, Hn, Dn);
        if (inside) {
            int x0, x1, y0, y1, z0, z1;
            double fx, fy, fz;
            clamp_split(x, Wn, x0, x1, fx);
            clamp_split(y, Hn, y0, y1, fy);
            clamp_split(z, Dn, z0, z1, fz);
            const long long o00 = ((long long)z0 * Hn + y0) * Wn, o01 = ((long long)z0 * Hn + y1) * Wn;
            const long long o10 = ((long long)z1 * Hn + y0) * Wn, o11 = ((long long)z1 * Hn + y1) * Wn;
            double acc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {                      // ITK component c (x, y, z) = phi channel 2 - c (w, h, d)
                const float* p = phi + (long long)(2 - c) * plane;
                const float sc = (float)((c == 0 ? Wn : c == 1 ? Hn : Dn) - 1);
                const float ia = c == 0 ? identity_coord(x0, inx) : c == 1 ? identity_coord(y0, iny) : identity_coord(z0, inz);
                const float ib = c == 0 ? identity_coord(x1, inx) : c == 1 ? identity_coord(y1, iny) : identity_coord(z1, inz);
                auto at = [&](bool zhi, bool yhi, bool xhi) {
                    const float id = c == 0 ? (xhi ? ib : ia) : c == 1 ? (yhi ? ib : ia) : (zhi ? ib : ia);
                    const long long row = zhi ? (yhi ? o11 : o10) : (yhi ? o01 : o00);
                    return itk_disp(p[row + (xhi ? x1 : x0)], id, sc);
                };
                acc[c] = lerp8(at, fx, fy, fz);
            }
            x += acc[0]; y += acc[1]; z += acc[2];
        }
        double ox, oy, oz;
        apply(n2o, x, y, z, ox, oy, oz);
        out[3 * i] = (float)ox; out[3 * i + 1] = (float)oy; out[3 * i + 2] = (float)oz;
        if (inside_out) inside_out[i] = inside ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int oai_transform_points_through_phi(const float* pts_dev, long long n, const float* phi_dev, int Dn, int Hn, int Wn,
                                     const oai_affine* point_to_net, const oai_affine* net_to_out, float* out_dev, unsigned char* inside_dev,
                                     void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_transform_points_through_phi: negative point count (%lld)", n);
    OAI_CHECK_ARG(Dn >= 2 && Hn >= 2 && Wn >= 2, "oai_transform_points_through_phi: every axis of phi needs at least 2 voxels (got %d x %d x %d)",
                  Dn, Hn, Wn);
    if (n == 0) return OAI_OK;
    OAI_CHECK_ARG(pts_dev && phi_dev && point_to_net && net_to_out && out_dev, "oai_transform_points_through_phi: null pointer");
    transform_points_kernel<<<grid_stride_blocks(n, kT), kT, 0, (hipStream_t)stream>>>(pts_dev, n, phi_dev, Dn, Hn, Wn, *point_to_net, *net_to_out,
                                                                                        out_dev, inside_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
