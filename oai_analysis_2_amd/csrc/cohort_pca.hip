// Cohort PCA for gfx950 (include/oai_hip.h, "Cohort PCA"; tests/cohort_pca_ref.py restates this file in numpy, operation for operation):
//   oai_cohort_whiten   values [N][V] (and a mask), mean [V], root weights [V] -> A [N][V] float64, and norm2 [N] on request
//   oai_rows_cross      A [n_a][V], B [n_b][V] -> C [n_a][n_b] = the ordered dot of every pair of rows: the Gram matrix, the hot kernel
//   oai_rows_combine    coef [K][N], rows [N][V] -> R [K][V] = the ordered combination of the rows: the modes, and the reconstruction
// The eigendecomposition between them is N x N and runs on the host.
//
// The order of every sum is the contract (the header states it): a dot is cut into chunks of kDotChunk = 512 vertices, a chunk is summed
// in ascending v into one accumulator, the chunk sums in ascending chunk index into another; a product, then an add, no FMA.  The vector
// fp64 MFMA would run this several times faster and is not used: its internal order cannot be restated.
//
// Shape of the cross kernel.  A 256-thread block owns a kTile x kTile = 64 x 64 tile of C; thread (ty, tx) of 16 x 16 owns the kOwn x kOwn
// = 4 x 4 entries of rows {32 h + 2 ty + e} x columns {32 h' + 2 tx + e'}: 16 chunk accumulators and, in the walk form, 16 totals.  A and B
// row slices of 64 rows x kSlice = 32 vertices go through LDS vertex-major (16 KB each, two buffers each: 64 KB, two blocks per CU), so
// that per vertex step a thread reads its four A and four B values as four ds_read_b128 for 16 multiplies and 16 adds.  A wave64 fp64
// operation occupies its SIMD for four cycles, a ds_read_b128 the LDS for four: per step 128 VALU cycles per SIMD against 4 waves x 16 LDS
// cycles per CU, so the fp64 VALU is the limiter by design.
//   Measured (profiles/cohort_pca.md): 27 % (split form, N = 200) and 29 % (walk form, N = 2000) of the fp64 issue rate at V = 30 002 --
//   not yet at that limit; the profile says what of the gap is known (a nearly empty second round of blocks) and what is supposed.
//   Banking.  A thread's two rows are adjacent so that they are one 16-byte read; the 16 tx of a read cover 256 contiguous bytes (all 64
//   banks once) and the ty are broadcasts.  The staging store is the transpose: thread t holds 8 consecutive vertices (quarter q = t % 4
//   of the slice) of row t / 4, and the 16 lanes that a ds_write_b64 serves together hold 4 rows x 4 quarters, which would meet in 8
//   banks; row r of vertex line vv is therefore stored at r ^ (4 (vv / 8)), which spreads the four quarters over the four 4-row groups of
//   their 16-row block and leaves a thread's pair of rows adjacent.  vv / 8 is a constant of the eight steps that are unrolled together.
//   The next slice's 16 global loads are issued before the 32 vertex steps of the current one and stored after them: one barrier per
//   slice.  Rows past n and vertices past V are staged as 0.0: an accumulator that starts at +0.0 never becomes -0.0 under round-to-
//   nearest, so adding the +0.0 products of the padding changes no bit of a sum.
// Two forms of the one body, chunk_sum().  Walk: a block per tile, all chunks, totals in registers.  Split: a block per (chunk, tile)
// writes the chunk sum to the workspace [chunk][tile][64 x 64] and finish_kernel adds them in ascending chunk index -- at N = 200 a 64 x 64
// tiling has ten upper-triangle tiles for 256 CUs.  With B == A the blocks below the diagonal leave at once and the others mirror their
// tile; a_iv * a_jv == a_jv * a_iv, so a diagonal tile is symmetric as computed.
#include "cohort.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kTile = 64;                          // edge of a block's tile of C
constexpr int kOwn = 4;                            // rows, and columns, per thread
constexpr int kSlice = 32;                         // vertices per LDS stage
constexpr int kSlices = kDotChunk / kSlice;        // stages per chunk
constexpr int kSplitMaxTiles = 256;                // the split form runs up to this many tiles (of the full rectangle)
constexpr int kCombineOwn = 4;                     // output rows per thread of the combine kernel
static_assert(kT == (kTile / kOwn) * (kTile / kOwn) && kT * 8 == kTile * kSlice && kDotChunk % kSlice == 0, "the tile's geometry");

// ---- oai_cohort_whiten -----------------------------------------------------------------------------------------------------------------
// A block per 256 consecutive vertices of one knee; the (knee, vertex block) pairs are walked with a grid stride.
__global__ void __launch_bounds__(kT) whiten_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, const double* __restrict__ mean,
                                                    const double* __restrict__ rw, long long N, long long V, long long vblocks, double* __restrict__ out) {
    for (long long blk = blockIdx.x; blk < N * vblocks; blk += gridDim.x) {
        const long long i = blk / vblocks, v = (blk % vblocks) * kT + threadIdx.x;
        if (v >= V) continue;
        const float y = Y[i * V + v];
        const double w = rw[v];
        const bool ok = (mask ? mask[i * V + v] != 0 : true) && y == y && w != 0.0;
        const double centred = (double)y - mean[v];
        out[i * V + v] = ok ? centred * w : 0.0;
    }
}

// norm2_i in the ordered-dot order: a block per knee (grid stride), thread t sums chunk base + t, thread 0 adds the 256 chunk sums in order.
__global__ void __launch_bounds__(kT) norm2_kernel(const double* __restrict__ A, long long N, long long V, double* __restrict__ norm2) {
    __shared__ double part[kT];
    const long long chunks = (V + kDotChunk - 1) / kDotChunk;
    for (long long i = blockIdx.x; i < N; i += gridDim.x) {
        double total = 0.0;
        for (long long base = 0; base < chunks; base += kT) {
            const long long c = base + threadIdx.x;
            double acc = 0.0;
            if (c < chunks) {
                const long long v1 = (c + 1) * kDotChunk < V ? (c + 1) * kDotChunk : V;
                for (long long v = c * kDotChunk; v < v1; ++v) {
                    const double a = A[i * V + v];
                    acc = acc + a * a;
                }
            }
            part[threadIdx.x] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int n = (int)(chunks - base < kT ? chunks - base : kT);
                for (int k = 0; k < n; ++k) total = total + part[k];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) norm2[i] = total;
    }
}

// ---- oai_rows_cross --------------------------------------------------------------------------------------------------------------------
struct CrossArgs {
    const double* A;
    const double* B;
    long long n_a, n_b, V;
    unsigned tiles_b;          // tiles along B; a tile's index is ti * tiles_b + tj
    int symmetric;             // B is A: tiles with tj < ti are skipped and the others mirrored
};

// this thread's share of one stage: 8 consecutive vertices from v0 + 8 (t % 4) of row row0 + t / 4, 0.0 outside the matrix
__device__ __forceinline__ void fetch(const double* __restrict__ X, long long n, long long V, long long row0, long long v0, double (&x)[8]) {
    const long long row = row0 + (threadIdx.x >> 2), v = v0 + (threadIdx.x & 3) * 8;
    const double* p = X + row * V + v;
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (row < n && v + k < V) ? p[k] : 0.0;
}

__device__ __forceinline__ void stage(double (*line)[kTile], const double (&x)[8]) {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
#pragma unroll
    for (int k = 0; k < 8; ++k) line[q * 8 + k][r ^ (q << 2)] = x[k];
}

// acc += the products of chunk c of this block's tile, in ascending v; every thread of the block calls it (it holds barriers)
__device__ __forceinline__ void chunk_sum(const CrossArgs& g, long long row_a, long long row_b, long long c, double (*sA)[kSlice][kTile],
                                          double (*sB)[kSlice][kTile], double (&acc)[kOwn][kOwn]) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long v_begin = c * kDotChunk;
    const long long left = g.V - v_begin;
    const int slices = left >= kDotChunk ? kSlices : (int)((left + kSlice - 1) / kSlice);
    double xa[8], xb[8];
    fetch(g.A, g.n_a, g.V, row_a, v_begin, xa);
    fetch(g.B, g.n_b, g.V, row_b, v_begin, xb);
    stage(sA[0], xa);
    stage(sB[0], xb);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < slices; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < slices;
        if (more) {
            fetch(g.A, g.n_a, g.V, row_a, v_begin + (long long)(s + 1) * kSlice, xa);
            fetch(g.B, g.n_b, g.V, row_b, v_begin + (long long)(s + 1) * kSlice, xb);
        }
        // eight vertex steps are unrolled at a time: unrolled over the whole slice, the compiler hoists every LDS read of the slice to its
        // top and spills (517 VGPRs to scratch); the swizzle is a constant of the eight
#pragma unroll 1
        for (int v8 = 0; v8 < kSlice; v8 += 8) {
            const int swz = (v8 >> 3) << 2;
#pragma unroll
            for (int vv = v8; vv < v8 + 8; ++vv) {
                const double2 a0 = *reinterpret_cast<const double2*>(&sA[cur][vv][(2 * ty) ^ swz]);
                const double2 a1 = *reinterpret_cast<const double2*>(&sA[cur][vv][(32 + 2 * ty) ^ swz]);
                const double2 b0 = *reinterpret_cast<const double2*>(&sB[cur][vv][(2 * tx) ^ swz]);
                const double2 b1 = *reinterpret_cast<const double2*>(&sB[cur][vv][(32 + 2 * tx) ^ swz]);
                const double a[kOwn] = {a0.x, a0.y, a1.x, a1.y}, b[kOwn] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < kOwn; ++i)
#pragma unroll
                    for (int j = 0; j < kOwn; ++j) acc[i][j] = acc[i][j] + a[i] * b[j];
            }
        }
        if (more) {
            stage(sA[cur ^ 1], xa);
            stage(sB[cur ^ 1], xb);
        }
        __syncthreads();
    }
}

// entry (i, j) of the thread's 4 x 4 within the tile: row 32 (i / 2) + 2 ty + i % 2, column 32 (j / 2) + 2 tx + j % 2
__device__ __forceinline__ int own_index(int t16, int k) { return 32 * (k >> 1) + 2 * t16 + (k & 1); }

__device__ __forceinline__ void write_tile(const CrossArgs& g, unsigned ti, unsigned tj, const double (&tot)[kOwn][kOwn], double* __restrict__ out) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < kOwn; ++i)
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            const long long row = (long long)ti * kTile + own_index(ty, i), col = (long long)tj * kTile + own_index(tx, j);
            if (row >= g.n_a || col >= g.n_b) continue;
            out[row * g.n_b + col] = tot[i][j];
            if (g.symmetric && ti != tj) out[col * g.n_b + row] = tot[i][j];
        }
}

__global__ void __launch_bounds__(kT, 2) cross_walk_kernel(CrossArgs g, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double sA[2][kSlice][kTile];
    __shared__ __attribute__((aligned(16))) double sB[2][kSlice][kTile];
    const unsigned ti = blockIdx.x / g.tiles_b, tj = blockIdx.x % g.tiles_b;
    if (g.symmetric && tj < ti) return;                                    // uniform over the block, before any barrier
    const long long chunks = (g.V + kDotChunk - 1) / kDotChunk;
    double tot[kOwn][kOwn] = {};
#pragma unroll 1
    for (long long c = 0; c < chunks; ++c) {
        double acc[kOwn][kOwn] = {};
        chunk_sum(g, (long long)ti * kTile, (long long)tj * kTile, c, sA, sB, acc);
#pragma unroll
        for (int i = 0; i < kOwn; ++i)
#pragma unroll
            for (int j = 0; j < kOwn; ++j) tot[i][j] = tot[i][j] + acc[i][j];
    }
    write_tile(g, ti, tj, tot, out);
}

// block = chunk * tiles + tile: the blocks that run together read the same vertices of all rows
__global__ void __launch_bounds__(kT, 2) cross_split_kernel(CrossArgs g, unsigned tiles, double* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) double sA[2][kSlice][kTile];
    __shared__ __attribute__((aligned(16))) double sB[2][kSlice][kTile];
    const unsigned tile = blockIdx.x % tiles;
    const long long c = blockIdx.x / tiles;
    const unsigned ti = tile / g.tiles_b, tj = tile % g.tiles_b;
    if (g.symmetric && tj < ti) return;
    double acc[kOwn][kOwn] = {};
    chunk_sum(g, (long long)ti * kTile, (long long)tj * kTile, c, sA, sB, acc);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double* slot = ws + ((long long)c * tiles + tile) * (kTile * kTile);
#pragma unroll
    for (int i = 0; i < kOwn; ++i)
#pragma unroll
        for (int j = 0; j < kOwn; ++j) slot[own_index(ty, i) * kTile + own_index(tx, j)] = acc[i][j];
}

// a thread per entry of a tile: the chunk sums in ascending chunk index, then the entry and its mirror
__global__ void __launch_bounds__(kT) cross_finish_kernel(CrossArgs g, unsigned tiles, long long chunks, const double* __restrict__ ws,
                                                         double* __restrict__ out) {
    const unsigned tile = blockIdx.x / (kTile * kTile / kT);
    const int e = (blockIdx.x % (kTile * kTile / kT)) * kT + threadIdx.x;
    const unsigned ti = tile / g.tiles_b, tj = tile % g.tiles_b;
    if (g.symmetric && tj < ti) return;
    const long long row = (long long)ti * kTile + e / kTile, col = (long long)tj * kTile + e % kTile;
    if (row >= g.n_a || col >= g.n_b) return;
    double total = 0.0;
    for (long long c = 0; c < chunks; ++c) total = total + ws[(c * tiles + tile) * (kTile * kTile) + e];
    out[row * g.n_b + col] = total;
    if (g.symmetric && ti != tj) out[col * g.n_b + row] = total;
}

static inline bool rows_ok(long long n) { return n >= 1 && n <= kMaxRows; }
static inline bool verts_ok(long long V) { return V >= 1 && V <= kMaxVerts; }

// tiles of the full rectangle, and whether the split form takes that many
static inline long long cross_tiles(long long n_a, long long n_b) { return (long long)cdiv(n_a, kTile) * cdiv(n_b, kTile); }
static inline size_t split_bytes(long long n_a, long long n_b, long long V) {
    return (size_t)cross_tiles(n_a, n_b) * (size_t)cdiv(V, kDotChunk) * (kTile * kTile * sizeof(double));
}

// ---- oai_rows_combine ------------------------------------------------------------------------------------------------------------------
// A thread owns one vertex and kCombineOwn output rows; block = row group * vblocks + vertex block.  The coefficients of a step are the
// same for the whole block and come through scalar loads; rows past n_out repeat the last one and are not stored.
__global__ void __launch_bounds__(kT) combine_kernel(const double* __restrict__ coef, const double* __restrict__ rows, long long K, long long N, long long V,
                                                     unsigned vblocks, double* __restrict__ out) {
    const long long c0 = (long long)(blockIdx.x / vblocks) * kCombineOwn;
    const long long v = (long long)(blockIdx.x % vblocks) * kT + threadIdx.x;
    if (v >= V) return;
    const double* k[kCombineOwn];
#pragma unroll
    for (int r = 0; r < kCombineOwn; ++r) k[r] = coef + (c0 + r < K ? c0 + r : K - 1) * N;
    double acc[kCombineOwn] = {};
    for (long long i = 0; i < N; ++i) {
        const double a = rows[i * V + v];
#pragma unroll
        for (int r = 0; r < kCombineOwn; ++r) acc[r] = acc[r] + k[r][i] * a;
    }
#pragma unroll
    for (int r = 0; r < kCombineOwn; ++r)
        if (c0 + r < K) out[(c0 + r) * V + v] = acc[r];
}

}  // namespace

extern "C" {

int oai_cohort_whiten(const float* values_dev, const unsigned char* mask_dev, const double* mean_dev, const double* root_weight_dev,
                      long long n_knees, long long n_verts, double* out_dev, double* norm2_dev, void* stream) {
    OAI_CHECK_ARG(n_knees >= 1 && n_knees <= kMaxKnees && verts_ok(n_verts),
                  "oai_cohort_whiten: needs n_knees 1 .. 2^24 and n_verts 1 .. 2^31-2 (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(values_dev, "oai_cohort_whiten: values_dev is a null pointer");
    OAI_CHECK_ARG(mean_dev, "oai_cohort_whiten: mean_dev is a null pointer");
    OAI_CHECK_ARG(root_weight_dev, "oai_cohort_whiten: root_weight_dev is a null pointer");
    OAI_CHECK_ARG(out_dev, "oai_cohort_whiten: out_dev is a null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const long long vblocks = cdiv(n_verts, kT);
    whiten_kernel<<<grid_stride_blocks(n_knees * vblocks, 1), kT, 0, st>>>(values_dev, mask_dev, mean_dev, root_weight_dev, n_knees, n_verts, vblocks,
                                                                          out_dev);
    OAI_CHECK_LAUNCH();
    if (norm2_dev) {
        norm2_kernel<<<grid_stride_blocks(n_knees, 1), kT, 0, st>>>(out_dev, n_knees, n_verts, norm2_dev);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

size_t oai_rows_cross_workspace_bytes(long long n_a, long long n_b, long long n_verts) {
    if (!rows_ok(n_a) || !rows_ok(n_b) || !verts_ok(n_verts) || cross_tiles(n_a, n_b) > kSplitMaxTiles) return 0;
    return split_bytes(n_a, n_b, n_verts);
}

int oai_rows_cross(const double* a_dev, long long n_a, const double* b_dev, long long n_b, long long n_verts, double* out_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream) {
    OAI_CHECK_ARG(rows_ok(n_a), "oai_rows_cross: n_a must be 1 .. 2^20 rows (got %lld)", n_a);
    OAI_CHECK_ARG(rows_ok(n_b), "oai_rows_cross: n_b must be 1 .. 2^20 rows (got %lld)", n_b);
    OAI_CHECK_ARG(verts_ok(n_verts), "oai_rows_cross: n_verts must be 1 .. 2^31-2 (got %lld)", n_verts);
    OAI_CHECK_ARG(a_dev, "oai_rows_cross: a_dev is a null pointer");
    OAI_CHECK_ARG(b_dev, "oai_rows_cross: b_dev is a null pointer");
    OAI_CHECK_ARG(out_dev, "oai_rows_cross: out_dev is a null pointer");
    const long long tiles = cross_tiles(n_a, n_b), chunks = cdiv(n_verts, kDotChunk);
    const bool split = workspace_dev && tiles <= kSplitMaxTiles;
    if (split) OAI_CHECK_WORKSPACE("oai_rows_cross", workspace_bytes, split_bytes(n_a, n_b, n_verts));
    OAI_CHECK_ARG(tiles < (1LL << 31), "oai_rows_cross: n_a = %lld by n_b = %lld is more tiles than one launch takes", n_a, n_b);
    const hipStream_t st = (hipStream_t)stream;
    const CrossArgs g = {a_dev, b_dev, n_a, n_b, n_verts, cdiv(n_b, kTile), (a_dev == b_dev && n_a == n_b) ? 1 : 0};
    if (!split) {
        cross_walk_kernel<<<(unsigned)tiles, kT, 0, st>>>(g, out_dev);
        OAI_CHECK_LAUNCH();
        return OAI_OK;
    }
    cross_split_kernel<<<(unsigned)(tiles * chunks), kT, 0, st>>>(g, (unsigned)tiles, (double*)workspace_dev);
    OAI_CHECK_LAUNCH();
    cross_finish_kernel<<<(unsigned)(tiles * (kTile * kTile / kT)), kT, 0, st>>>(g, (unsigned)tiles, chunks, (const double*)workspace_dev, out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_rows_combine(const double* coef_dev, const double* rows_dev, long long n_out, long long n_rows, long long n_verts, double* out_dev,
                     void* stream) {
    OAI_CHECK_ARG(rows_ok(n_out), "oai_rows_combine: n_out must be 1 .. 2^20 rows (got %lld)", n_out);
    OAI_CHECK_ARG(rows_ok(n_rows), "oai_rows_combine: n_rows must be 1 .. 2^20 rows (got %lld)", n_rows);
    OAI_CHECK_ARG(verts_ok(n_verts), "oai_rows_combine: n_verts must be 1 .. 2^31-2 (got %lld)", n_verts);
    OAI_CHECK_ARG(coef_dev, "oai_rows_combine: coef_dev is a null pointer");
    OAI_CHECK_ARG(rows_dev, "oai_rows_combine: rows_dev is a null pointer");
    OAI_CHECK_ARG(out_dev, "oai_rows_combine: out_dev is a null pointer");
    const unsigned vblocks = cdiv(n_verts, kT);
    const long long blocks = (long long)vblocks * cdiv(n_out, kCombineOwn);
    OAI_CHECK_ARG(blocks < (1LL << 31), "oai_rows_combine: n_out = %lld and n_verts = %lld are more than one launch takes: combine a shorter span", n_out,
                  n_verts);
    combine_kernel<<<(unsigned)blocks, kT, 0, (hipStream_t)stream>>>(coef_dev, rows_dev, n_out, n_rows, n_verts, vblocks, out_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
