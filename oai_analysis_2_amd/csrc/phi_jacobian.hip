// Registration QC for gfx950: the Jacobian determinant of the dense map phi with its fold count, and the overlap counts of two
// thresholded probability maps (Dice, cartilage volume).
//
//   oai_phi_jacobian    one determinant per cell (z,y,x), z in [1,D), y in [1,H), x in [1,W): the backward-difference stencil of
//                       icon_registration.losses.flips, restated from memory and unpinned (icon_registration is absent), on the
//                       DISPLACEMENT u = (phi - identity) * (n - 1) rebuilt in fp32 by the function that phi_to_disp_kernel (csrc/warp.hip)
//                       and transform_points_kernel (csrc/mesh_transform.hip) call (itk_disp, csrc/phi_field.h):  J[r][k] = delta_rk + (u_r(p) - u_r(p - e_k)).
//                       The float32 identity coordinates do not difference exactly, so the raw-phi form of the identity map reads
//                       det in [0.999977, 1.0000048] at (80,192,192); the displacement form reads exactly 1.
//   oai_mask_overlap    |A|, |B|, |A and B| and the non-finite positions of two float32 arrays under `value > threshold`
//
// Both are memory-bound streaming reductions.  phi_jacobian_kernel: x is the lane (a wave = 64 consecutive cells of one row, coalesced),
// a block is 4 rows x 8 cells along z; each thread walks its z-run with the previous plane's displacement kept in registers, and the
// x - 1 and y - 1 neighbours are lines that the same wave / the wave next to it in the block has just fetched (L1, at a block edge L2):
// every phi value leaves HBM once, apart from the one plane in eight that two z-chunks share.  fp64 arithmetic with contraction off,
// written so that a numpy restatement performs the same operations in the same order (tests/phi_jacobian_ref.py).  Measured
// (profiles/registration_qc.md): 16 us at 80x192x192, a third of the memory rate -- the 65 fp64 instructions per cell weigh about as
// much as the 35 MB; requesting a thread's whole z-run up front changed nothing.  oai_mask_overlap runs at the memory rate.
// Reductions: per-thread in z order, then the ordered block reduction of csrc/ordered_reduce.h (one slot per block in the workspace, a
// second one-block kernel over the slots).  No atomics, and the block count depends on the shape only: the stats are bit-reproducible
// and the same whether or not the map is written.
#include "common.h"

#include <cstdint>

#pragma clang fp contract(off)

#include "ordered_reduce.h"
#include "phi_field.h"      // after the pragma: compiled with contraction off here (see its leading comment)

namespace {

using namespace oai;

constexpr int kT = 256;                       // threads per block
constexpr int kTX = 64, kTY = 4, kZC = 8;     // phi_jacobian_kernel's block of cells: x (one wave per row), y, z
constexpr int kJP = 6;                        // doubles per block partial: folds, non-finite, min, max, sum, sum of squares
constexpr int kMP = 4;                        // counts per block partial of mask_overlap_kernel
constexpr long long kMaskBlocks = 2048;       // 256 CUs x 8 blocks: grid-stride beyond that

struct JacAcc {
    double v[kJP];
    __device__ __forceinline__ void clear() {
        v[0] = 0.0; v[1] = 0.0; v[2] = INFINITY; v[3] = -INFINITY; v[4] = 0.0; v[5] = 0.0;
    }
    __device__ __forceinline__ void merge(const double* o) {      // this (the earlier cells) on the left of every sum
        v[0] = v[0] + o[0]; v[1] = v[1] + o[1]; v[2] = fmin(v[2], o[2]); v[3] = fmax(v[3], o[3]); v[4] = v[4] + o[4]; v[5] = v[5] + o[5];
    }
};

__global__ void __launch_bounds__(kT)
phi_jacobian_kernel(const float* __restrict__ phi, int D, int H, int W, int nbx, int nby, float* __restrict__ det_out, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kJP];
    const long long plane = (long long)D * H * W;
    const double inz = 1.0 / (D - 1), iny = 1.0 / (H - 1), inx = 1.0 / (W - 1);
    const float sz = (float)(D - 1), sy = (float)(H - 1), sx = (float)(W - 1);
    const long long b = blockIdx.x;
    const int bx = (int)(b % nbx), by = (int)((b / nbx) % nby), bz = (int)(b / ((long long)nbx * nby));
    const int x = 1 + bx * kTX + (int)(threadIdx.x & 63), y = 1 + by * kTY + (int)(threadIdx.x >> 6);
    const int z0 = 1 + bz * kZC, z1 = min(z0 + kZC, D);
    // ITK component c (x, y, z) = phi channel 2 - c (w, h, d)
    auto disp = [&](int zz, int yy, int xx, const float idz, double* u) {
        const long long o = ((long long)zz * H + yy) * W + xx;
        u[0] = itk_disp(phi[2 * plane + o], identity_coord(xx, inx), sx);
        u[1] = itk_disp(phi[plane + o], identity_coord(yy, iny), sy);
        u[2] = itk_disp(phi[o], idz, sz);
    };
    JacAcc acc;
    acc.clear();
    if (x < W && y < H) {
        double below[3];                                           // u(p - e_z): the previous step's u(p)
        disp(z0 - 1, y, x, identity_coord(z0 - 1, inz), below);
        for (int z = z0; z < z1; ++z) {
            const float idz = identity_coord(z, inz);
            double c[3], ax[3], ay[3];
            disp(z, y, x, idz, c);
            disp(z, y, x - 1, idz, ax);
            disp(z, y - 1, x, idz, ay);
            const double J00 = 1.0 + (c[0] - ax[0]), J01 = c[0] - ay[0], J02 = c[0] - below[0];
            const double J10 = c[1] - ax[1], J11 = 1.0 + (c[1] - ay[1]), J12 = c[1] - below[1];
            const double J20 = c[2] - ax[2], J21 = c[2] - ay[2], J22 = 1.0 + (c[2] - below[2]);
            const double det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20);
            if (det_out) det_out[((long long)(z - 1) * (H - 1) + (y - 1)) * (W - 1) + (x - 1)] = (float)det;
            if (isfinite(det)) {
                if (det < 0.0) acc.v[0] = acc.v[0] + 1.0;
                acc.v[2] = fmin(acc.v[2], det);
                acc.v[3] = fmax(acc.v[3], det);
                acc.v[4] = acc.v[4] + det;
                acc.v[5] = acc.v[5] + det * det;
            } else {
                acc.v[1] = acc.v[1] + 1.0;
            }
            below[0] = c[0]; below[1] = c[1]; below[2] = c[2];
        }
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kJP; ++i) partials[b * kJP + i] = acc.v[i];
}

// one block: the slots in runs, then the same tree (csrc/ordered_reduce.h)
__global__ void __launch_bounds__(kT)
phi_jacobian_finish_kernel(const double* __restrict__ partials, long long nb, double cells, double* __restrict__ stats) {
    __shared__ double lds[kT / 64][kJP];
    JacAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        stats[0] = cells;
        for (int i = 0; i < kJP; ++i) stats[1 + i] = acc.v[i];
    }
}

struct MaskAcc {
    unsigned long long v[kMP];                 // |A|, |B|, |A and B|, positions with a non-finite value
    __device__ __forceinline__ void clear() { v[0] = 0; v[1] = 0; v[2] = 0; v[3] = 0; }
    __device__ __forceinline__ void merge(const unsigned long long* o) { v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3]; }
    template <bool HAS_B>
    __device__ __forceinline__ void add(float a, float b, float thr) {
        const bool fa = finite_f32(a), fb = !HAS_B || finite_f32(b);
        const bool ina = fa && a > thr, inb = HAS_B && fb && b > thr;
        v[0] += ina; v[1] += inb; v[2] += (ina && inb); v[3] += !(fa && fb);
    }
};

// nvec float4 pieces (0 when a pointer is not 16-byte aligned), then the remaining elements one by one; both grid-stride
template <bool HAS_B>
__global__ void __launch_bounds__(kT)
mask_overlap_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, long long nvec, float thr,
                    unsigned long long* __restrict__ partials) {
    __shared__ unsigned long long lds[kT / 64][kMP];
    MaskAcc acc;
    acc.clear();
    const long long t = (long long)blockIdx.x * kT + threadIdx.x, stride = (long long)gridDim.x * kT;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    for (long long i = t; i < nvec; i += stride) {
        const float4 va = a4[i];
        const float4 vb = HAS_B ? b4[i] : va;
        acc.add<HAS_B>(va.x, vb.x, thr); acc.add<HAS_B>(va.y, vb.y, thr); acc.add<HAS_B>(va.z, vb.z, thr); acc.add<HAS_B>(va.w, vb.w, thr);
    }
    for (long long i = 4 * nvec + t; i < n; i += stride) acc.add<HAS_B>(a[i], HAS_B ? b[i] : 0.0f, thr);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kMP; ++i) partials[(long long)blockIdx.x * kMP + i] = acc.v[i];
}

__global__ void __launch_bounds__(kT)
mask_overlap_finish_kernel(const unsigned long long* __restrict__ partials, int nb, long long* __restrict__ counts) {
    __shared__ unsigned long long lds[kT / 64][kMP];
    MaskAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < kMP; ++k) counts[k] = (long long)acc.v[k];
}

struct JacGrid {
    long long nbx, nby, nbz, nb;
};

JacGrid jac_grid(int D, int H, int W) {
    JacGrid g;
    g.nbx = (W - 1 + kTX - 1) / kTX;
    g.nby = (H - 1 + kTY - 1) / kTY;
    g.nbz = (D - 1 + kZC - 1) / kZC;
    g.nb = g.nbx * g.nby * g.nbz;
    return g;
}

long long mask_blocks(long long n) {
    const long long pieces = (n + 3) / 4, blocks = (pieces + kT - 1) / kT;
    return blocks > kMaskBlocks ? kMaskBlocks : blocks;
}

}  // namespace

extern "C" {

size_t oai_phi_jacobian_workspace_bytes(int D, int H, int W) {
    if (D < 2 || H < 2 || W < 2) return 0;
    oai::Ws ws(nullptr);
    ws.take<double>((size_t)jac_grid(D, H, W).nb * kJP);
    return ws.off;
}

int oai_phi_jacobian(const float* phi_dev, int D, int H, int W, float* det_out_dev, void* workspace_dev, size_t workspace_bytes,
                     double* stats_dev, void* stream) {
    OAI_CHECK_ARG(D >= 2 && H >= 2 && W >= 2, "oai_phi_jacobian: every axis of phi needs at least 2 voxels (got %d x %d x %d)", D, H, W);
    OAI_CHECK_ARG(phi_dev && workspace_dev && stats_dev, "oai_phi_jacobian: null pointer");
    const JacGrid g = jac_grid(D, H, W);
    OAI_CHECK_ARG(g.nb <= 0x7fffffffLL, "oai_phi_jacobian: %d x %d x %d is too large for one launch", D, H, W);
    OAI_CHECK_WORKSPACE("oai_phi_jacobian", workspace_bytes, oai_phi_jacobian_workspace_bytes(D, H, W));
    oai::Ws ws(workspace_dev);
    double* partials = ws.take<double>((size_t)g.nb * kJP);
    const hipStream_t st = (hipStream_t)stream;
    phi_jacobian_kernel<<<(unsigned)g.nb, kT, 0, st>>>(phi_dev, D, H, W, (int)g.nbx, (int)g.nby, det_out_dev, partials);
    OAI_CHECK_LAUNCH();
    const double cells = (double)(D - 1) * (double)(H - 1) * (double)(W - 1);
    phi_jacobian_finish_kernel<<<1, kT, 0, st>>>(partials, g.nb, cells, stats_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_mask_overlap_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    oai::Ws ws(nullptr);
    ws.take<unsigned long long>((size_t)mask_blocks(n) * kMP);
    return ws.off;
}

int oai_mask_overlap(const float* a_dev, const float* b_dev, long long n, float threshold, void* workspace_dev, size_t workspace_bytes,
                     long long* counts_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0, "oai_mask_overlap: negative element count (%lld)", n);
    OAI_CHECK_ARG(counts_dev && (n == 0 || (a_dev && workspace_dev)), "oai_mask_overlap: null pointer");
    OAI_CHECK_WORKSPACE("oai_mask_overlap", workspace_bytes, oai_mask_overlap_workspace_bytes(n));
    const hipStream_t st = (hipStream_t)stream;
    const int nb = (int)mask_blocks(n);
    unsigned long long* partials = (unsigned long long*)workspace_dev;
    if (nb) {
        const bool aligned = (uintptr_t)a_dev % 16 == 0 && (uintptr_t)b_dev % 16 == 0;
        const long long nvec = aligned ? n / 4 : 0;
        if (b_dev)
            mask_overlap_kernel<true><<<(unsigned)nb, kT, 0, st>>>(a_dev, b_dev, n, nvec, threshold, partials);
        else
            mask_overlap_kernel<false><<<(unsigned)nb, kT, 0, st>>>(a_dev, nullptr, n, nvec, threshold, partials);
        OAI_CHECK_LAUNCH();
    }
    mask_overlap_finish_kernel<<<1, kT, 0, st>>>(partials, nb, counts_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
