// Surface smoothing for gfx950 (include/oai_hip.h, "Surface smoothing"; tests/graph_smooth_ref.py restates the definition in numpy):
// K sweeps of normalised neighbourhood averaging of every row of a float64 tile on a weighted CSR vertex graph, under a validity mask
// that each sweep reads and writes.  An invalid entry is skipped by a select, never multiplied by 0.
//   oai_graph_smooth     transpose in, K sweep launches that ping-pong between two buffers of the workspace, transpose out
//
// fp64 without contraction.  The order IS the contract: per (row, vertex) one numerator and one denominator, the vertex itself first,
// then its neighbours in ascending CSR position.  Every output element is formed by one thread from the previous sweep's buffer alone,
// so the bits do not depend on the launch geometry; there are no atomics of any kind.
//
// Shape, and why.  The tile arrives [R][V], row (knee) major.  A sweep gathers, per vertex, the values of its ~6 neighbours: in [R][V]
// a wave of 64 consecutive vertices would gather 64 scattered 8-byte words per neighbour slot and row -- one 64-byte line fetched for
// every 8 bytes used.  So the tile is transposed ONCE on entry into [V][R] (and once back on exit): a wave then covers 64 consecutive
// rows of one vertex, the gather of neighbour j is one contiguous run x[j][r .. r + 63] of 512 bytes, its mask a run of 64 bytes, and
// the CSR offsets, the neighbour index and the weight are the same address in (almost) every lane of the wave -- a broadcast.  The
// two transposes cost about two sweeps' traffic against the K ~ 70 of a 5 mm FWHM.  With few rows (R = 1: one knee, an impulse)
// [V][R] is [R][V] again and the gather is scattered, which at that size does not matter.
//   Thread = one (vertex, row) element of the flat [V][R] index, grid-stride; vertex and row advance by a fixed (quotient, remainder)
//     step, so there is one 64-bit division per thread and none per element.
//   The workspace holds two value buffers (float64) and two mask buffers (uint8) of R * V each.  An invalid entry holds +0.0 in the
//     workspace, whatever the caller stored under its 0 mask byte: it is loaded (the loads are unconditional, so that they can all be
//     in flight together) and then dropped by the select.
// Measured (profiles/surface_smoothing.md).
#include "cohort.h"
#include "csr_graph.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kSmoothT = 256;
constexpr int kTile = 32;                          // the transposes move 32 x 32 tiles through LDS
constexpr int kGather = 8;                        // neighbour slots whose loads are in flight together
constexpr int kMaxSweeps = 4096;

struct SmoothWs {
    double* x[2];
    unsigned char* m[2];
    size_t bytes;
    SmoothWs(const void* base, long long rows, long long V) {
        Ws ws(base);
        for (int k = 0; k < 2; ++k) x[k] = ws.take<double>((size_t)(rows * V));
        for (int k = 0; k < 2; ++k) m[k] = ws.take<unsigned char>((size_t)(rows * V));
        bytes = ws.off;
    }
};

// values [R][V] (+ mask or null) -> x [V][R], m [V][R]; an invalid entry becomes +0.0 / 0.  blockDim = (32, 8).
__global__ void __launch_bounds__(kTile * 8) smooth_in_kernel(const double* __restrict__ values, const unsigned char* __restrict__ mask, long long R,
                                                              long long V, double* __restrict__ x, unsigned char* __restrict__ m) {
    __shared__ double tx[kTile][kTile + 1];
    __shared__ unsigned char tm[kTile][kTile + 1];
    const long long v0 = (long long)blockIdx.x * kTile, r0 = (long long)blockIdx.y * kTile;
    for (int k = threadIdx.y; k < kTile; k += 8) {
        const long long r = r0 + k, v = v0 + threadIdx.x;
        if (r < R && v < V) {
            const unsigned char ok = mask ? (mask[r * V + v] != 0) : 1;
            tm[k][threadIdx.x] = ok;
            tx[k][threadIdx.x] = ok ? values[r * V + v] : 0.0;
        }
    }
    __syncthreads();
    for (int k = threadIdx.y; k < kTile; k += 8) {
        const long long v = v0 + k, r = r0 + threadIdx.x;
        if (r < R && v < V) {
            x[v * R + r] = tx[threadIdx.x][k];
            m[v * R + r] = tm[threadIdx.x][k];
        }
    }
}

// x [V][R], m [V][R] -> out_values [R][V] and, unless null, out_mask [R][V].  blockDim = (32, 8).
__global__ void __launch_bounds__(kTile * 8) smooth_out_kernel(const double* __restrict__ x, const unsigned char* __restrict__ m, long long R, long long V,
                                                               double* __restrict__ out_values, unsigned char* __restrict__ out_mask) {
    __shared__ double tx[kTile][kTile + 1];
    __shared__ unsigned char tm[kTile][kTile + 1];
    const long long v0 = (long long)blockIdx.x * kTile, r0 = (long long)blockIdx.y * kTile;
    for (int k = threadIdx.y; k < kTile; k += 8) {
        const long long v = v0 + k, r = r0 + threadIdx.x;
        if (r < R && v < V) {
            tx[k][threadIdx.x] = x[v * R + r];
            tm[k][threadIdx.x] = m[v * R + r];
        }
    }
    __syncthreads();
    for (int k = threadIdx.y; k < kTile; k += 8) {
        const long long r = r0 + k, v = v0 + threadIdx.x;
        if (r < R && v < V) {
            out_values[r * V + v] = tx[threadIdx.x][k];
            if (out_mask) out_mask[r * V + v] = tm[threadIdx.x][k];
        }
    }
}

// One sweep, (x, m) -> (xn, mn), all four [V][R].  A thread starts at flat element blockIdx.x * 256 + threadIdx.x and advances by the
// grid's size, which the host passes as step_v vertices and step_r < R rows.
__global__ void __launch_bounds__(kSmoothT) smooth_sweep_kernel(const double* __restrict__ x, const unsigned char* __restrict__ m, long long R, long long V,
                                                                const int* __restrict__ offsets, const int* __restrict__ neighbours, long long n_nbrs,
                                                                const double* __restrict__ edge_w, const double* __restrict__ self_w, int fill,
                                                                long long step_v, long long step_r, double* __restrict__ xn,
                                                                unsigned char* __restrict__ mn) {
    const long long first = (long long)blockIdx.x * kSmoothT + threadIdx.x;
    long long i = first / R, r = first % R;
    for (; i < V; i += step_v, r += step_r) {
        if (r >= R) {
            r -= R;
            if (++i >= V) break;
        }
        const long long at = i * R + r;
        const CsrSlots slots = csr_slots(offsets, i, n_nbrs);
        const long long a = slots.a, b = slots.b;
        const bool mi = m[at] != 0;
        const double xi = x[at], sw = self_w ? self_w[i] : 1.0;
        double num = 0.0, den = 0.0;
        {
            const double p = sw * xi, n1 = num + p, d1 = den + sw;
            num = mi ? n1 : num;
            den = mi ? d1 : den;
        }
        // kGather slots at a time: their indices and weights are loaded together, then their values and masks, and only the adds run
        // one after the other -- a slot's two dependent loads are paid once per group, not once per neighbour (a hub of degree 200
        // would otherwise be a chain of 400 load latencies).  A slot past the end or with a neighbour out of range reads the
        // vertex' own entry and is dropped by the select.  Of csrc/csr_graph.h this loop shares the slot range only, not the test of
        // a neighbour: a vertex among its own neighbours counts here, and the range test feeds a select, not a branch.
        for (long long e0 = a; e0 < b; e0 += kGather) {
            double w[kGather], xj[kGather];
            int j[kGather];
            unsigned char mj[kGather];
            long long from[kGather];
#pragma unroll
            for (int u = 0; u < kGather; ++u) {
                const long long e = e0 + u < b ? e0 + u : e0;
                j[u] = neighbours[e];
                w[u] = edge_w[e];
            }
#pragma unroll
            for (int u = 0; u < kGather; ++u) {                            // no branch from here on: bitwise logic and selects only
                const bool in = (e0 + u < b) & (j[u] >= 0) & ((long long)j[u] < V);
                from[u] = (long long)((unsigned long long)(unsigned)(in ? j[u] : (int)i) * (unsigned)R) + r;
                xj[u] = x[from[u]];
                mj[u] = m[from[u]] & (in ? 0xff : 0);
            }
#pragma unroll
            for (int u = 0; u < kGather; ++u) {
                const double p = w[u] * xj[u], n1 = num + p, d1 = den + w[u];
                num = mj[u] ? n1 : num;                                    // a select: what lies under a 0 mask reaches no sum
                den = mj[u] ? d1 : den;
            }
        }
        const bool ok = (fill || mi) && den > 0.0;
        xn[at] = ok ? num / den : 0.0;
        mn[at] = ok ? 1 : 0;
    }
}

}  // namespace

extern "C" {

size_t oai_graph_smooth_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return SmoothWs(nullptr, n_rows, n_verts).bytes;
}

int oai_graph_smooth(const double* values_dev, const unsigned char* mask_dev, long long n_rows, long long n_verts, const int* offsets_dev,
                     const int* neighbours_dev, long long n_neighbours, const double* edge_weight_dev, const double* self_weight_dev, int sweeps,
                     int fill, void* workspace_dev, size_t workspace_bytes, double* out_values_dev, unsigned char* out_mask_dev, void* stream) {
    OAI_CHECK_GRAPH_TILE("oai_graph_smooth", n_rows, n_verts, n_neighbours);
    OAI_CHECK_ARG(sweeps >= 1 && sweeps <= kMaxSweeps, "oai_graph_smooth: sweeps must be 1 .. 4096, got %d", sweeps);
    OAI_CHECK_ARG(fill == 0 || fill == 1, "oai_graph_smooth: fill must be 0 (keep) or 1 (fill), got %d", fill);
    OAI_CHECK_ARG(workspace_dev && out_values_dev && values_dev && offsets_dev && (n_neighbours == 0 || (neighbours_dev && edge_weight_dev)),
                  "oai_graph_smooth: null pointer");
    OAI_CHECK_WORKSPACE("oai_graph_smooth", workspace_bytes, oai_graph_smooth_workspace_bytes(n_rows, n_verts));
    const SmoothWs ws(workspace_dev, n_rows, n_verts);
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(cdiv(n_verts, kTile), cdiv(n_rows, kTile)), tile_threads(kTile, 8);
    smooth_in_kernel<<<tiles, tile_threads, 0, st>>>(values_dev, mask_dev, n_rows, n_verts, ws.x[0], ws.m[0]);
    OAI_CHECK_LAUNCH();
    const long long total = n_rows * n_verts;
    const unsigned blocks = grid_stride_blocks(total, kSmoothT);
    const long long step = (long long)blocks * kSmoothT;
    for (int s = 0; s < sweeps; ++s) {
        smooth_sweep_kernel<<<blocks, kSmoothT, 0, st>>>(ws.x[s & 1], ws.m[s & 1], n_rows, n_verts, offsets_dev, neighbours_dev, n_neighbours,
                                                         edge_weight_dev, self_weight_dev, fill, step / n_rows, step % n_rows, ws.x[(s + 1) & 1],
                                                         ws.m[(s + 1) & 1]);
        OAI_CHECK_LAUNCH();
    }
    smooth_out_kernel<<<tiles, tile_threads, 0, st>>>(ws.x[sweeps & 1], ws.m[sweeps & 1], n_rows, n_verts, out_values_dev, out_mask_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
