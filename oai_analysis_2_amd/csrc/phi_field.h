// The arithmetic of the dense map phi, shared by every kernel that reads it: warp.hip (phi_to_disp_kernel, resample_kernel,
// resample_maps_kernel, the identity map of the warps), mesh_transform.hip (transform_points_kernel) and phi_jacobian.hip
// (phi_jacobian_kernel).  That these kernels rebuild ONE displacement from phi is what the fused resample, the pushed meshes and the
// fold count rest on, so the rebuild is written here once (itk_disp) and nowhere else.
//
// Contraction: this header carries NO `#pragma clang fp contract` of its own, and must not get one.  The library is compiled with
// -ffp-contract=on; mesh_transform.hip and phi_jacobian.hip switch contraction off at file scope because their numpy restatements
// (tests/mesh_transform_ref.py, tests/phi_jacobian_ref.py) round every product and sum, while warp.hip leaves it on (its fp32 gathers
// are contracted).  Include this header AFTER the including file's pragma: each translation unit then compiles these functions in its
// own mode.  As compiled today no fp64 chain of warp.hip holds a fused multiply-add (profiles/phi_field_refactor.md).
#pragma once
#include "common.h"

namespace oai {

// mermaidlite.identity_map: float32(index * spacing) with spacing = 1/(n-1) in float64
__device__ __forceinline__ float identity_coord(int i, double inv_nm1) {
    return (float)((double)i * inv_nm1);
}

__device__ __forceinline__ void apply(const oai_affine& t, double x, double y, double z, double& ox, double& oy, double& oz) {
    ox = t.A[0] * x + t.A[1] * y + t.A[2] * z + t.b[0];
    oy = t.A[3] * x + t.A[4] * y + t.A[5] * z + t.b[1];
    oz = t.A[6] * x + t.A[7] * y + t.A[8] * z + t.b[2];
}

// c clamped to [0, n-1] (a NaN clamps to 0): corners i0 <= i1 <= n-1 and the weight of i1
__device__ __forceinline__ void clamp_split(double c, int n, int& i0, int& i1, double& f) {
    c = fmin(fmax(c, 0.0), (double)(n - 1));
    const double fl = floor(c);
    i0 = (int)fl;
    i1 = min(i0 + 1, n - 1);
    f = c - fl;
}

// The half-open test of ITK's buffered region on a continuous index (false for a NaN).  A flag set under the tests, not `return a &&
// b ...`: this spelling compiles to the instructions of the tests written in place in all five uses, the plain return does not (it
// merges two of the six compares in resample_maps_kernel; profiles/phi_field_refactor.md).
__device__ __forceinline__ bool inside_buffer(double x, double y, double z, int nx, int ny, int nz) {
    bool in = false;
    if (x >= -0.5 && x < nx - 0.5 && y >= -0.5 && y < ny - 0.5 && z >= -0.5 && z < nz - 0.5) in = true;
    return in;
}

// One component of the displacement the ITK transform holds, at one lattice point: phi's value there, the identity coordinate of the
// point along that component's axis and (float)(n - 1) of that axis.  fp32 like the reference -- (phi - ident), then *= (shape - 1),
// then .double().  ITK component c (x, y, z) is phi channel 2 - c (w, h, d).
__device__ __forceinline__ double itk_disp(float phi_value, float identity, float nm1) {
    return (double)((phi_value - identity) * nm1);
}

// Trilinear lerp in fp64 of the eight corner values v(zhi, yhi, xhi) (0 = the lower corner of that axis, 1 = the upper): x, then y, then
// z.  The corners come through a callable, not as eight arguments, so that each is fetched where the chain first uses it, as when
// the chain was written out in the kernels: with eight arguments all loads are hoisted ahead of the arithmetic and
// transform_points_kernel takes two more VGPRs.
template <class V>
__device__ __forceinline__ double lerp8(V&& v, double fx, double fy, double fz) {
    const double c00 = v(0, 0, 0) * (1 - fx) + v(0, 0, 1) * fx;
    const double c01 = v(0, 1, 0) * (1 - fx) + v(0, 1, 1) * fx;
    const double c10 = v(1, 0, 0) * (1 - fx) + v(1, 0, 1) * fx;
    const double c11 = v(1, 1, 0) * (1 - fx) + v(1, 1, 1) * fx;
    return (c00 * (1 - fy) + c01 * fy) * (1 - fz) + (c10 * (1 - fy) + c11 * fy) * fz;
}

}  // namespace oai
