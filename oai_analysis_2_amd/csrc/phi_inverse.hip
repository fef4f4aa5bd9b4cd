// The inverse of the registration's dense map phi for gfx950: patient (A) points taken back to the atlas (B).
//
// phi provides one direction, atlas -> patient (csrc/mesh_transform.hip).  In network index space that map is
//   T(x) = x + (inside_buffer(x) ? u(x) : 0),   u = the trilinear lerp (x, then y, then z) of itk_disp at the 8 clamped corners,
// and this file solves T(x) = y for x, per point, by Newton's method on the trilinear interpolant.  It is what
// itk.Transform.GetInverseTransform means for a displacement field -- a numerical inverse of the map that is held, exact up to a stated
// residual -- restated from ITK's documented behaviour and unpinned (ITK is absent), like the resample and the point push.  It is NOT
// the network's own phi_BA (a second registration with the inputs swapped, which only approximates the inverse).
//   oai_inverse_points_through_phi   one thread per point, grid-stride: affine in, solve, affine out
//   oai_invert_phi                   the dense inverse psi on phi's own lattice, in phi's own storage convention: psi is a phi, and the
//                                    resample, the point push and the Jacobian read it unchanged; plus the solver's statistics
//
// One __device__ solver serves both.  Newton, not the plain fixed point x <- y - u(x): that diverges wherever phi stretches by a factor
// of 2 or more (|grad u| >= 1), Newton converges quadratically from x = y on every field without folds that was tried.  The step falls
// back to the fixed point where |det(I + grad u)| <= 1e-3, the neighbourhood of a fold, where the Newton step is unbounded.
// Everything is fp64 with contraction off, through the functions of phi_field.h, written so that a numpy restatement performs the same
// operations in the same order (tests/phi_inverse_ref.py): iterates, status and iteration counts are reproducible to the bit.
//
// Latency-bound gather: 24 scattered 4-byte loads per iteration per point out of a field that sits in L2 / Infinity Cache after the
// registration.  No LDS outside the statistics' block reduction, no atomics.  The statistics are reduced like oai_phi_jacobian's, by
// the ordered block reduction of csrc/ordered_reduce.h: one slot per block in the workspace and a second one-block kernel over the
// slots; the block count depends on the shape only.
#include "common.h"

#pragma clang fp contract(off)

#include "ordered_reduce.h"
#include "phi_field.h"      // after the pragma: compiled with contraction off here (see its leading comment)

namespace {

using namespace oai;

constexpr int kT = 256;                       // threads per block
constexpr int kSP = 5;                        // doubles per block partial: unconverged, converged outside, max |r|, sum of iterations, max iterations
constexpr double kDetMin = 1e-3;              // |det(I + grad u)| at or below this: a fixed-point step instead of Newton's

struct Field {
    const float* phi;
    int Dn, Hn, Wn;
    long long plane;
    double inz, iny, inx;
    __device__ __forceinline__ Field(const float* p, int D, int H, int W)
        : phi(p), Dn(D), Hn(H), Wn(W), plane((long long)D * H * W), inz(1.0 / (D - 1)), iny(1.0 / (H - 1)), inx(1.0 / (W - 1)) {}
};

// u(x) and G[c][k] = d u_c / d x_k of the trilinear interpolant, from the 8 clamped corners.  d is lerp8's value (the bits of
// transform_points_kernel's displacement); G is the exact gradient of the same polynomial inside the cell.  An axis clamped at its
// upper end has i0 == i1 and so a zero column; one clamped at its lower end (coordinate in [-0.5, 0)) has its column set to zero, the
// interpolant being constant along it there.
__device__ __forceinline__ void disp_and_gradient(const Field& F, double x, double y, double z, double* d, double (*G)[3]) {
    int x0, x1, y0, y1, z0, z1;
    double fx, fy, fz;
    clamp_split(x, F.Wn, x0, x1, fx);
    clamp_split(y, F.Hn, y0, y1, fy);
    clamp_split(z, F.Dn, z0, z1, fz);
    const long long o00 = ((long long)z0 * F.Hn + y0) * F.Wn, o01 = ((long long)z0 * F.Hn + y1) * F.Wn;
    const long long o10 = ((long long)z1 * F.Hn + y0) * F.Wn, o11 = ((long long)z1 * F.Hn + y1) * F.Wn;
    const bool lowx = x < 0.0, lowy = y < 0.0, lowz = z < 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                      // ITK component c (x, y, z) = phi channel 2 - c (w, h, d)
        const float* p = F.phi + (long long)(2 - c) * F.plane;
        const float sc = (float)((c == 0 ? F.Wn : c == 1 ? F.Hn : F.Dn) - 1);
        const float ia = c == 0 ? identity_coord(x0, F.inx) : c == 1 ? identity_coord(y0, F.iny) : identity_coord(z0, F.inz);
        const float ib = c == 0 ? identity_coord(x1, F.inx) : c == 1 ? identity_coord(y1, F.iny) : identity_coord(z1, F.inz);
        double v[8];                                   // corner (zhi, yhi, xhi) at 4 zhi + 2 yhi + xhi
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool zhi = k & 4, yhi = k & 2, xhi = k & 1;
            const float id = c == 0 ? (xhi ? ib : ia) : c == 1 ? (yhi ? ib : ia) : (zhi ? ib : ia);
            const long long row = zhi ? (yhi ? o11 : o10) : (yhi ? o01 : o00);
            v[k] = itk_disp(p[row + (xhi ? x1 : x0)], id, sc);
        }
        d[c] = lerp8([&](bool zhi, bool yhi, bool xhi) { return v[4 * zhi + 2 * yhi + xhi]; }, fx, fy, fz);
        // d/dx: the x-differences of the four edges, lerped along y, then z
        const double gx = ((v[1] - v[0]) * (1 - fy) + (v[3] - v[2]) * fy) * (1 - fz) + ((v[5] - v[4]) * (1 - fy) + (v[7] - v[6]) * fy) * fz;
        // d/dy and d/dz: from lerp8's own x-lerps
        const double c00 = v[0] * (1 - fx) + v[1] * fx, c01 = v[2] * (1 - fx) + v[3] * fx;
        const double c10 = v[4] * (1 - fx) + v[5] * fx, c11 = v[6] * (1 - fx) + v[7] * fx;
        const double gy = (c01 - c00) * (1 - fz) + (c11 - c10) * fz;
        const double gz = (c10 * (1 - fy) + c11 * fy) - (c00 * (1 - fy) + c01 * fy);
        G[c][0] = lowx ? 0.0 : gx;
        G[c][1] = lowy ? 0.0 : gy;
        G[c][2] = lowz ? 0.0 : gz;
    }
}

struct Solved {
    double x, y, z;        // the preimage (status 1, 2), or the start point y itself (status 0)
    double resid;          // max_c |r_c| at convergence; 0 for status 0
    int iters;             // evaluations of T that were made
    int status;            // 1 = converged inside the buffer, 2 = converged outside it (T is the identity there), 0 = not converged
};

__device__ __forceinline__ Solved solve(const Field& F, double yx, double yy, double yz, int max_iter, double tol) {
    Solved s;
    s.x = yx; s.y = yy; s.z = yz; s.resid = 0.0; s.iters = 0; s.status = 0;
    double x = yx, y = yy, z = yz;
    for (int it = 0; it < max_iter; ++it) {
        s.iters = it + 1;
        const bool inside = inside_buffer(x, y, z, F.Wn, F.Hn, F.Dn);
        double d[3] = {0.0, 0.0, 0.0};
        double G[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        if (inside) disp_and_gradient(F, x, y, z, d, G);
        const double r0 = (x + d[0]) - yx, r1 = (y + d[1]) - yy, r2 = (z + d[2]) - yz;
        const double rmax = fmax(fmax(fabs(r0), fabs(r1)), fabs(r2));
        if (rmax <= tol) {                             // (false for a NaN residual)
            s.x = x; s.y = y; s.z = z; s.resid = rmax; s.status = inside ? 1 : 2;
            break;
        }
        const double J00 = 1.0 + G[0][0], J01 = G[0][1], J02 = G[0][2];
        const double J10 = G[1][0], J11 = 1.0 + G[1][1], J12 = G[1][2];
        const double J20 = G[2][0], J21 = G[2][1], J22 = 1.0 + G[2][2];
        const double det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20);   // as phi_jacobian_kernel
        double s0 = r0, s1 = r1, s2 = r2;              // the fixed-point step
        if (fabs(det) > kDetMin) {                     // Newton: s = J^-1 r by the adjugate
            s0 = (((J11 * J22 - J12 * J21) * r0 + (J02 * J21 - J01 * J22) * r1) + (J01 * J12 - J02 * J11) * r2) / det;
            s1 = (((J12 * J20 - J10 * J22) * r0 + (J00 * J22 - J02 * J20) * r1) + (J02 * J10 - J00 * J12) * r2) / det;
            s2 = (((J10 * J21 - J11 * J20) * r0 + (J01 * J20 - J00 * J21) * r1) + (J00 * J11 - J01 * J10) * r2) / det;
        }
        if (!(isfinite(s0) && isfinite(s1) && isfinite(s2))) break;
        x -= s0; y -= s1; z -= s2;
    }
    return s;
}

__global__ void __launch_bounds__(kT)
inverse_points_kernel(const float* __restrict__ pts, long long n, const float* __restrict__ phi, int Dn, int Hn, int Wn, oai_affine p2n,
                      oai_affine n2o, int max_iter, double tol, float* __restrict__ out, unsigned char* __restrict__ status_out) {
    const Field F(phi, Dn, Hn, Wn);
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        double yx, yy, yz;
        apply(p2n, (double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], yx, yy, yz);
        const Solved s = solve(F, yx, yy, yz, max_iter, tol);
        double ox, oy, oz;
        apply(n2o, s.x, s.y, s.z, ox, oy, oz);
        out[3 * i] = (float)ox; out[3 * i + 1] = (float)oy; out[3 * i + 2] = (float)oz;
        if (status_out) status_out[i] = (unsigned char)s.status;
    }
}

struct InvAcc {
    double v[kSP];
    __device__ __forceinline__ void clear() {
        for (int i = 0; i < kSP; ++i) v[i] = 0.0;
    }
    __device__ __forceinline__ void merge(const double* o) {      // this (the earlier points) on the left of every sum
        v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = fmax(v[2], o[2]); v[3] = v[3] + o[3]; v[4] = fmax(v[4], o[4]);
    }
};

// one thread per lattice point, x fastest: block b owns points [b kT, (b + 1) kT)
__global__ void __launch_bounds__(kT)
invert_phi_kernel(const float* __restrict__ phi, int D, int H, int W, int max_iter, double tol, float* __restrict__ psi,
                  unsigned char* __restrict__ status_out, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kSP];
    const Field F(phi, D, H, W);
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    InvAcc acc;
    acc.clear();
    if (i < F.plane) {
        const int xi = (int)(i % W), yi = (int)((i / W) % H), zi = (int)(i / ((long long)W * H));
        const Solved s = solve(F, (double)xi, (double)yi, (double)zi, max_iter, tol);
        psi[2 * F.plane + i] = (float)(s.x * F.inx);             // phi's storage: channel 2 - c holds component c in [0,1] units
        psi[F.plane + i] = (float)(s.y * F.iny);
        psi[i] = (float)(s.z * F.inz);
        if (status_out) status_out[i] = (unsigned char)s.status;
        acc.v[0] = s.status == 0 ? 1.0 : 0.0;
        acc.v[1] = s.status == 2 ? 1.0 : 0.0;
        acc.v[2] = s.resid;
        acc.v[3] = (double)s.iters;
        acc.v[4] = (double)s.iters;
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < kSP; ++k) partials[(long long)blockIdx.x * kSP + k] = acc.v[k];
}

// one block: the slots in runs, then the same tree (csrc/ordered_reduce.h)
__global__ void __launch_bounds__(kT)
invert_phi_finish_kernel(const double* __restrict__ partials, long long nb, double points, double* __restrict__ stats) {
    __shared__ double lds[kT / 64][kSP];
    InvAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        stats[0] = points;
        for (int k = 0; k < kSP; ++k) stats[1 + k] = acc.v[k];
    }
}

long long dense_blocks(int D, int H, int W) { return ((long long)D * H * W + kT - 1) / kT; }

}  // namespace

extern "C" {

int oai_inverse_points_through_phi(const float* pts_dev, long long n, const float* phi_dev, int Dn, int Hn, int Wn,
                                   const oai_affine* point_to_net, const oai_affine* net_to_out, int max_iter, double tol, float* out_dev,
                                   unsigned char* status_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_inverse_points_through_phi: negative point count (%lld)", n);
    OAI_CHECK_ARG(Dn >= 2 && Hn >= 2 && Wn >= 2, "oai_inverse_points_through_phi: every axis of phi needs at least 2 voxels (got %d x %d x %d)",
                  Dn, Hn, Wn);
    OAI_CHECK_ARG(max_iter >= 1, "oai_inverse_points_through_phi: max_iter must be at least 1 (got %d)", max_iter);
    OAI_CHECK_ARG(tol > 0.0, "oai_inverse_points_through_phi: tol must be positive (got %g)", tol);
    if (n == 0) return OAI_OK;
    OAI_CHECK_ARG(pts_dev && phi_dev && point_to_net && net_to_out && out_dev, "oai_inverse_points_through_phi: null pointer");
    inverse_points_kernel<<<grid_stride_blocks(n, kT), kT, 0, (hipStream_t)stream>>>(pts_dev, n, phi_dev, Dn, Hn, Wn, *point_to_net, *net_to_out,
                                                                                      max_iter, tol, out_dev, status_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_invert_phi_workspace_bytes(int D, int H, int W) {
    if (D < 2 || H < 2 || W < 2) return 0;
    oai::Ws ws(nullptr);
    ws.take<double>((size_t)dense_blocks(D, H, W) * kSP);
    return ws.off;
}

int oai_invert_phi(const float* phi_dev, int D, int H, int W, int max_iter, double tol, float* psi_out_dev, unsigned char* status_out_dev,
                   void* workspace_dev, size_t workspace_bytes, double* stats_dev, void* stream) {
    OAI_CHECK_ARG(D >= 2 && H >= 2 && W >= 2, "oai_invert_phi: every axis of phi needs at least 2 voxels (got %d x %d x %d)", D, H, W);
    OAI_CHECK_ARG(max_iter >= 1, "oai_invert_phi: max_iter must be at least 1 (got %d)", max_iter);
    OAI_CHECK_ARG(tol > 0.0, "oai_invert_phi: tol must be positive (got %g)", tol);
    OAI_CHECK_ARG(phi_dev && psi_out_dev && workspace_dev && stats_dev, "oai_invert_phi: null pointer");
    OAI_CHECK_ARG(psi_out_dev != phi_dev, "oai_invert_phi: psi_out_dev may not alias phi_dev");
    const long long nb = dense_blocks(D, H, W);
    OAI_CHECK_ARG(nb <= 0x7fffffffLL, "oai_invert_phi: %d x %d x %d is too large for one launch", D, H, W);
    OAI_CHECK_WORKSPACE("oai_invert_phi", workspace_bytes, oai_invert_phi_workspace_bytes(D, H, W));
    oai::Ws ws(workspace_dev);
    double* partials = ws.take<double>((size_t)nb * kSP);
    const hipStream_t st = (hipStream_t)stream;
    invert_phi_kernel<<<(unsigned)nb, kT, 0, st>>>(phi_dev, D, H, W, max_iter, tol, psi_out_dev, status_out_dev, partials);
    OAI_CHECK_LAUNCH();
    invert_phi_finish_kernel<<<1, kT, 0, st>>>(partials, nb, (double)D * (double)H * (double)W, stats_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
