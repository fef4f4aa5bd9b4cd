// Segmentation-shape QC for gfx950: 3-D connected-component labelling of a thresholded map or a byte mask (or of its complement) under
// 6, 18 or 26 connectivity, with the per-voxel component size and a twelve-integer summary (include/oai_hip.h, "Segmentation-shape QC").
//
// Union-find over the voxels with THE SMALLEST LINEAR INDEX OF A COMPONENT AS ITS REPRESENTATIVE.  parent[i] <= i always, a link only
// ever moves to a smaller index of the same component (integer atomicMin), so whatever order the workgroups ran in, every tree ends
// rooted at the minimum index of its component: the result is a function of the input alone.  The raster-order numbering is then the
// exclusive scan of the root flags.
//
//   cc_brick_kernel      a brick of 4 x 4 x 64 voxels per block: membership, union-find in LDS over the 3 / 9 / 13 neighbours that precede
//                        a voxel in raster order (the other half is some other voxel's preceding half), then every voxel's parent = its
//                        brick-local root as a global index.  Clears the per-root accumulators; counts the non-finite values.
//   cc_seam_kernel       every pair of neighbouring voxels that lie in DIFFERENT bricks (faces; for 18 and 26 also the pairs across a
//                        brick edge or corner): find both roots by reads and, only where they differ, link the larger under the smaller
//                        with a returning atomicMin.  Paths walked are shortened (each node under its grandparent) with non-returning atomicMin.
//   cc_flatten_kernel    parent[i] = root(i); size and border flag of every component into acc[root]: one atomic per run of
//                        x-adjacent lanes of a wave that share a root, and one per block for the runs of the block's first component
//   cc_count_kernel      per 1024 voxels: the number of roots, and one slot of the summary's partial figures
//   cc_finish_kernel     one block: exclusive scan of the per-block root counts and the summary, slots in the order of ordered_reduce.h
//   cc_rank_kernel       labels[root] = 1 + its rank in raster order; 0 off the set
//   cc_gather_kernel     labels[i] = labels[root(i)], size[i] = size of root(i)
//
// Stream order is the only grid-wide synchronisation: no kernel waits for another workgroup, nothing is read back by the host.  Every
// loop is bounded: a find walks strictly decreasing parents, and each turn of a union's loop strictly lowers the larger of its two
// indices.  Integer atomics only (atomicMin, atomicAdd, atomicOr); no floating-point value is reduced.
#include "common.h"

#include <climits>
#include <cmath>
#include <cstdint>

#include "ordered_reduce.h"

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kBZ = 4, kBY = 4, kBX = 64;          // the brick: one 64-voxel row per wave instruction, 16 rows
constexpr int kBrick = kBZ * kBY * kBX;            // 1024 voxels, four per thread
constexpr int kSeg = 1024;                         // voxels per block of the count / rank kernels: 256 consecutive per wave
constexpr int kMaxAxis = 32767;
constexpr long long kMaxVoxels = 2147483647LL;     // indices are int32
constexpr int kSlots = 10;                         // long long per block partial of the summary
constexpr unsigned kBorderBit = 0x80000000u;       // acc[root] = voxel count (< 2^31) | border flag
constexpr int kOut = -1;                           // parent of a voxel that is not in the labelled set

// the neighbours that precede a voxel in raster order: 3 faces, then 6 edges, then 4 corners -- 6 / 18 / 26 connectivity use the
// first 3 / 9 / 13
__constant__ signed char kBack[13][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0},
                                         {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1}, {-1, -1, 0}, {-1, 1, 0},
                                         {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__host__ __device__ inline int back_count(int connectivity) { return connectivity == 6 ? 3 : (connectivity == 18 ? 9 : 13); }

// ---- union-find in LDS -----------------------------------------------------------------------------------------------------------------
// (relaxed atomic loads and not volatile ones: a volatile access through the pointer stays a flat load, these become ds_read)
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(const int* lab, int a) {
    for (int p; (p = lds_ld(lab + a)) != a;) a = p;        // p < a: terminates
    return a;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }      // a > b
        const int old = atomicMin(&lab[a], b);
        if (old == a) break;                               // a was a root and now hangs under b
        a = old;                                           // a hung under `old` < a already: join old and b instead
    }
}

// ---- union-find in global memory -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(const int* parent, int a) {
    for (int p; (p = ld(parent + a)) != a;) a = p;
    return a;
}

// The root of a's tree as memory holds it: the walk reads through the XCD's L2, which is not coherent with the other XCDs' atomics, so
// the node it ends at is confirmed by an atomic that changes nothing (parent[r] <= r) and returns the word from the memory side.
__device__ __forceinline__ int g_find_confirmed(int* parent, int a) {
    int r = g_find(parent, a);
    for (int p; (p = g_min(parent + r, r)) != r;) r = g_find(parent, p);       // p < r: terminates
    return r;
}

// find with path splitting: every node on the way is hung under its grandparent (atomicMin: a link never moves up).  Only under its
// OWN ancestor, read in this same walk: a root found by an earlier walk may by now belong to another tree than the node does (the
// two joined only by some thread's pending union), and moving the node's subtree there would make that union find nothing to do
// and leave the rest of the node's old tree cut off.
__device__ __forceinline__ int g_find_compress(int* parent, int a) {
    for (;;) {
        const int p = ld(parent + a);
        if (p == a) return a;
        const int gp = ld(parent + p);                 // gp <= p < a: terminates
        if (gp != p) g_min(parent + a, gp);
        a = p;
    }
}

__device__ __forceinline__ void g_union(int* parent, int a, int b) {
    a = g_find_compress(parent, a);
    b = g_find_compress(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = g_min(parent + a, b);
        if (old == a) break;
        a = old;
    }
}

// ---- the brick -------------------------------------------------------------------------------------------------------------------------
struct CountAcc {
    unsigned long long v[1];
    __device__ __forceinline__ void clear() { v[0] = 0; }
    __device__ __forceinline__ void merge(const unsigned long long* o) { v[0] += o[0]; }
};

__global__ void __launch_bounds__(kT)
cc_brick_kernel(const float* __restrict__ map, const unsigned char* __restrict__ mask, int D, int H, int W, int nbx, int nby, float thr,
                int complement, int n_back, int* __restrict__ parent, unsigned* __restrict__ acc, unsigned long long* __restrict__ nonfinite) {
    __shared__ int lab[kBrick];
    __shared__ unsigned long long red[kT / 64][1];
    const int bx = (int)(blockIdx.x % (unsigned)nbx), by = (int)((blockIdx.x / (unsigned)nbx) % (unsigned)nby),
              bz = (int)(blockIdx.x / ((unsigned)nbx * (unsigned)nby));
    const int lx = threadIdx.x & (kBX - 1), ly = threadIdx.x >> 6;
    const int x = bx * kBX + lx, y = by * kBY + ly;
    const bool col = x < W && y < H;
    CountAcc bad;
    bad.clear();
#pragma unroll
    for (int lz = 0; lz < kBZ; ++lz) {
        const int z = bz * kBZ + lz, l = (lz * kBY + ly) * kBX + lx;
        bool in = false;
        if (col && z < D) {
            const int g = (z * H + y) * W + x;
            if (map) {
                const float v = map[g];
                in = in_set(v, thr);
                bad.v[0] += !finite_f32(v);
            } else {
                in = mask[g] != 0;
            }
            if (complement) in = !in;
            st(acc + g, 0u);
        }
        lab[l] = in ? l : kOut;
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < kBZ; ++lz) {
        const int l = (lz * kBY + ly) * kBX + lx;
        if (lab[l] == kOut) continue;
        for (int k = 0; k < n_back; ++k) {
            const int qz = lz + kBack[k][0], qy = ly + kBack[k][1], qx = lx + kBack[k][2];
            if (qz < 0 || qy < 0 || qy >= kBY || qx < 0 || qx >= kBX) continue;            // in another brick: cc_seam_kernel
            const int q = (qz * kBY + qy) * kBX + qx;
            if (lds_ld(lab + q) != kOut) lds_union(lab, l, q);
        }
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < kBZ; ++lz) {
        const int z = bz * kBZ + lz, l = (lz * kBY + ly) * kBX + lx;
        if (!(col && z < D)) continue;
        int root = kOut;
        if (lab[l] != kOut) {
            const int r = lds_find(lab, l);                                                // raster order inside a brick is raster order outside
            root = ((bz * kBZ + r / (kBY * kBX)) * H + by * kBY + (r / kBX) % kBY) * W + bx * kBX + r % kBX;
        }
        st(parent + ((z * H + y) * W + x), root);
    }
    if (map) {
        block_reduce<kT>(bad, red);
        if (threadIdx.x == 0 && bad.v[0]) atomicAdd(nonfinite, bad.v[0]);
    }
}

// one thread per voxel: its preceding neighbours that lie in another brick
__global__ void __launch_bounds__(kT) cc_seam_kernel(int D, int H, int W, int n_back, int* parent) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= (long long)D * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)H * W));
    const int lx = x & (kBX - 1), ly = y & (kBY - 1), lz = z & (kBZ - 1);
    if (lx != 0 && lx != kBX - 1 && ly != 0 && ly != kBY - 1 && lz != 0) return;           // every preceding neighbour is in this brick
    if (ld(parent + i) == kOut) return;
    for (int k = 0; k < n_back; ++k) {
        const int dz = kBack[k][0], dy = kBack[k][1], dx = kBack[k][2];
        const int qz = z + dz, qy = y + dy, qx = x + dx;
        if (qz < 0 || qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
        const int mz = lz + dz, my = ly + dy, mx = lx + dx;
        if (mz >= 0 && my >= 0 && my < kBY && mx >= 0 && mx < kBX) continue;               // the same brick: merged in LDS
        const int q = (qz * H + qy) * W + qx;
        if (ld(parent + q) != kOut) g_union(parent, (int)i, q);
    }
}

// Lanes hold consecutive voxels.  A run of lanes with one root adds once: the lane that starts the run adds the run's length, and sets
// the border bit if any voxel of the run has an index 0 or n - 1 on some axis.  A block takes 1024 consecutive voxels.  The runs that
// belong to the component of the block's first voxel -- inside a large component nearly all of them -- are summed in LDS and reach the
// root's word as one atomicAdd per block: a component of m voxels draws about m / 1024 global atomics on its one word, not m / 64.
__global__ void __launch_bounds__(kT) cc_flatten_kernel(int D, int H, int W, int* parent, unsigned* acc) {
    __shared__ int first_root;
    __shared__ unsigned first_acc;
    const long long n = (long long)D * H * W, base = (long long)blockIdx.x * kSeg;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        first_root = ld(parent + base) != kOut ? g_find_confirmed(parent, (int)base) : kOut;      // base < n: the grid is ceil(n / 1024)
        first_acc = 0;
    }
    __syncthreads();
    const int r0 = first_root;
#pragma unroll
    for (int k = 0; k < kSeg / kT; ++k) {
        const long long i = base + k * kT + threadIdx.x;
        int root = kOut;
        bool border = false;
        if (i < n && ld(parent + i) != kOut) {
            root = g_find(parent, (int)i);
            const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((long long)H * W));
            border = x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1;
        }
        // runs by the root as read; the lane that starts a run confirms it (the block's first root is confirmed already) and the
        // run takes what that lane found
        const int before = __shfl_up(root, 1, 64);
        const bool head = lane == 0 || before != root;
        const unsigned long long heads = __ballot(head);
        if (head && root != kOut && root != r0) root = g_find_confirmed(parent, root);
        const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1));       // bit 0 is always set: lane 0 is a head
        const int from_head = __shfl(root, 63 - __clzll((long long)upto), 64);
        if (root != kOut) {
            root = from_head;
            st(parent + i, root);
        }
        const unsigned long long borders = __ballot(border);
        if (head && root != kOut) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);      // the next run starts at the lowest set bit
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << lane;
            const unsigned add = (unsigned)len | ((borders & run) ? kBorderBit : 0u);      // at most 1024 voxels per block: bit 31 stays the flag
            if (root == r0) {
                atomicAdd(&first_acc, add & ~kBorderBit);
                if (add & kBorderBit) atomicOr(&first_acc, kBorderBit);
            } else {
                atomicAdd(acc + root, add & ~kBorderBit);
                if (add & kBorderBit) atomicOr(acc + root, kBorderBit);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && r0 != kOut) {
        atomicAdd(acc + r0, first_acc & ~kBorderBit);
        if (first_acc & kBorderBit) atomicOr(acc + r0, kBorderBit);
    }
}

// ---- numbering and the summary ---------------------------------------------------------------------------------------------------------
// [0] voxels of the set  [1] roots  [2] largest size  [3] its root (the smallest on a tie; LLONG_MAX: none)  [4] second largest size
// [5], [6] components below min_voxels and their voxels  [7], [8] components that touch the border and their voxels  [9] spare
struct SumAcc {
    long long v[kSlots];
    __device__ __forceinline__ void clear() {
        for (int i = 0; i < kSlots; ++i) v[i] = 0;
        v[3] = LLONG_MAX;
    }
    __device__ __forceinline__ void take(long long size, long long root, long long min_voxels, bool border) {
        const long long o[kSlots] = {0, 1, size, root, 0, size < min_voxels ? 1 : 0, size < min_voxels ? size : 0, border ? 1 : 0, border ? size : 0, 0};
        merge(o);
    }
    __device__ __forceinline__ void merge(const long long* o) {
        v[0] += o[0]; v[1] += o[1]; v[5] += o[5]; v[6] += o[6]; v[7] += o[7]; v[8] += o[8]; v[9] += o[9];
        if (o[2] > v[2] || (o[2] == v[2] && o[3] < v[3])) {            // the two largest of {v[2] >= v[4], o[2] >= o[4]} as a multiset
            v[4] = v[2] > o[4] ? v[2] : o[4];
            v[2] = o[2];
            v[3] = o[3];
        } else {
            v[4] = v[4] > o[2] ? v[4] : o[2];
        }
    }
};

// block b: voxels [1024 b, 1024 b + 1024); wave w its 256 consecutive ones in four steps of 64
__global__ void __launch_bounds__(kT)
cc_count_kernel(const int* __restrict__ parent, const unsigned* __restrict__ acc, long long n, long long min_voxels, int* __restrict__ counts,
                long long* __restrict__ partials) {
    __shared__ long long lds[kT / 64][kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kSeg + wave * 256;
    SumAcc s;
    s.clear();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + k * 64 + lane;
        if (i >= n) continue;
        const int p = parent[i];
        s.v[0] += p != kOut;
        if (p == (int)i) {
            const unsigned a = acc[i];
            s.take((long long)(a & ~kBorderBit), i, min_voxels, (a & kBorderBit) != 0);
        }
    }
    block_reduce<kT>(s, lds);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = (int)s.v[1];
        for (int i = 0; i < kSlots; ++i) partials[(long long)blockIdx.x * kSlots + i] = s.v[i];
    }
}

// one block.  Thread t owns the run of consecutive blocks of reduce_slots: their partials merged in index order, their root counts
// scanned; thread 0 scans the 256 run totals and writes the summary.  The largest component's label is its root's rank + 1: the
// roots in front of it inside its own 1024-voxel block are counted here, so that the label needs neither labels_dev nor size_dev.
__global__ void __launch_bounds__(kT)
cc_finish_kernel(const int* __restrict__ parent, const int* __restrict__ counts, const long long* __restrict__ partials, long long nb, long long n,
                 const unsigned long long* __restrict__ nonfinite, int* __restrict__ offsets, long long* __restrict__ summary) {
    __shared__ long long lds[kT / 64][kSlots];
    __shared__ long long run_total[kT];
    __shared__ unsigned long long red[kT / 64][1];
    __shared__ long long top_root, top_base;
    SumAcc s;
    reduce_slots<kT>(partials, nb, s);
    const long long per = (nb + kT - 1) / kT;
    const long long i0 = min(per * (long long)threadIdx.x, nb), i1 = min(i0 + per, nb);
    run_total[threadIdx.x] = s.v[1];
    block_reduce<kT>(s, lds);                                          // (its barrier also publishes run_total)
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int t = 0; t < kT; ++t) { const long long c = run_total[t]; run_total[t] = sum; sum += c; }
        top_root = s.v[1] ? s.v[3] : -1;
        summary[0] = n;
        summary[1] = s.v[0];
        summary[2] = s.v[1];
        summary[3] = s.v[2];
        summary[5] = s.v[4];
        summary[6] = s.v[5]; summary[7] = s.v[6]; summary[8] = s.v[7]; summary[9] = s.v[8];
        summary[10] = (long long)*nonfinite;
        summary[11] = 0;
    }
    __syncthreads();
    const long long top = top_root, top_block = top >= 0 ? top / kSeg : -1;
    long long at = run_total[threadIdx.x];
    for (long long b = i0; b < i1; ++b) {
        offsets[b] = (int)at;
        if (b == top_block) top_base = at;
        at += counts[b];
    }
    CountAcc before;
    before.clear();
    if (top >= 0)
        for (long long j = top_block * kSeg + threadIdx.x; j < top; j += kT) before.v[0] += parent[j] == (int)j;
    block_reduce<kT>(before, red);                                     // (its barrier also publishes top_base)
    if (threadIdx.x == 0) summary[4] = top >= 0 ? top_base + (long long)before.v[0] + 1 : 0;
}

// the roots of block b get offsets[b] + 1, + 2, ... in index order; every other voxel of the set is written by cc_gather_kernel
__global__ void __launch_bounds__(kT)
cc_rank_kernel(const int* __restrict__ parent, const int* __restrict__ offsets, long long n, int* __restrict__ labels) {
    __shared__ int wave_roots[kT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kSeg + wave * 256;
    bool is_root[4];
    int rank[4], seen = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + k * 64 + lane;
        is_root[k] = i < n && parent[i] == (int)i;
        const unsigned long long m = __ballot(is_root[k]);
        rank[k] = seen + __popcll(m & ((1ull << lane) - 1));
        seen += __popcll(m);
    }
    if (lane == 0) wave_roots[wave] = seen;
    __syncthreads();
    int first = offsets[blockIdx.x] + 1;
    for (int w = 0; w < wave; ++w) first += wave_roots[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + k * 64 + lane;
        if (i < n && (is_root[k] || parent[i] == kOut)) labels[i] = is_root[k] ? first + rank[k] : 0;
    }
}

__global__ void __launch_bounds__(kT)
cc_gather_kernel(const int* __restrict__ parent, const unsigned* __restrict__ acc, long long n, int* labels, int* __restrict__ size) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int p = parent[i];
    if (labels && p != kOut && p != (int)i) labels[i] = labels[p];     // labels[p] is a root's: written by cc_rank_kernel, not here
    if (size) size[i] = p == kOut ? 0 : (int)(acc[p] & ~kBorderBit);
}

// ---- oai_component_sizes ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
cc_sizes_kernel(const int* __restrict__ labels, long long n, long long n_components, unsigned long long* sizes) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int label = 0;
    if (i < n) {
        label = labels[i];
        if (label < 0 || (long long)label > n_components) label = 0;
    }
    const int before = __shfl_up(label, 1, 64);
    const bool head = lane == 0 || before != label;
    const unsigned long long heads = __ballot(head);
    if (head && label != 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        atomicAdd(sizes + (label - 1), (unsigned long long)(above ? __ffsll((long long)above) : 64 - lane));
    }
}

bool shape_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= kMaxAxis && H <= kMaxAxis && W <= kMaxAxis && (long long)D * H * W <= kMaxVoxels;
}

struct CcWs {
    int* parent;
    unsigned* acc;
    int *counts, *offsets;
    long long* partials;
    unsigned long long* nonfinite;
    long long blocks;
    size_t bytes;
    CcWs(void* workspace, int D, int H, int W) {
        Ws ws(workspace);
        const size_t n = (size_t)D * H * W;
        blocks = (long long)((n + kSeg - 1) / kSeg);
        parent = ws.take<int>(n);
        acc = ws.take<unsigned>(n);
        counts = ws.take<int>((size_t)blocks);
        offsets = ws.take<int>((size_t)blocks);
        partials = ws.take<long long>((size_t)blocks * kSlots);
        nonfinite = ws.take<unsigned long long>(1);
        bytes = ws.off;
    }
};

}  // namespace

extern "C" {

size_t oai_label_components_workspace_bytes(int D, int H, int W) {
    if (!shape_ok(D, H, W)) return 0;
    return CcWs(nullptr, D, H, W).bytes;
}

int oai_label_components(const float* map_dev, const unsigned char* mask_dev, int D, int H, int W, float threshold, int complement,
                         int connectivity, long long min_voxels, int* labels_dev, int* size_dev, void* workspace_dev, size_t workspace_bytes,
                         long long* summary_dev, void* stream) {
    OAI_CHECK_ARG(D >= 1 && H >= 1 && W >= 1 && D <= kMaxAxis && H <= kMaxAxis && W <= kMaxAxis,
                  "oai_label_components: every axis must be in [1, %d] (got %d x %d x %d)", kMaxAxis, D, H, W);
    OAI_CHECK_ARG((long long)D * H * W <= kMaxVoxels, "oai_label_components: %d x %d x %d is more than 2^31 - 1 voxels", D, H, W);
    OAI_CHECK_ARG((map_dev != nullptr) != (mask_dev != nullptr), "oai_label_components: exactly one of map_dev and mask_dev must be given");
    OAI_CHECK_ARG(summary_dev && workspace_dev, "oai_label_components: null pointer");
    OAI_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "oai_label_components: connectivity must be 6, 18 or 26, got %d",
                  connectivity);
    OAI_CHECK_ARG(min_voxels >= 0, "oai_label_components: negative min_voxels (%lld)", min_voxels);
    OAI_CHECK_ARG(!map_dev || !std::isnan(threshold), "oai_label_components: the threshold is NaN");
    OAI_CHECK_WORKSPACE("oai_label_components", workspace_bytes, oai_label_components_workspace_bytes(D, H, W));
    const CcWs ws(workspace_dev, D, H, W);
    const hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)D * H * W;
    const int n_back = back_count(connectivity);
    const unsigned nbx = cdiv(W, kBX), nby = cdiv(H, kBY), nbz = cdiv(D, kBZ), per_voxel = cdiv(n, kT);
    OAI_CHECK_HIP(hipMemsetAsync(ws.nonfinite, 0, sizeof(unsigned long long), st));
    cc_brick_kernel<<<nbx * nby * nbz, kT, 0, st>>>(map_dev, mask_dev, D, H, W, (int)nbx, (int)nby, threshold, complement != 0, n_back, ws.parent,
                                                    ws.acc, ws.nonfinite);
    OAI_CHECK_LAUNCH();
    cc_seam_kernel<<<per_voxel, kT, 0, st>>>(D, H, W, n_back, ws.parent);
    OAI_CHECK_LAUNCH();
    cc_flatten_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(D, H, W, ws.parent, ws.acc);
    OAI_CHECK_LAUNCH();
    cc_count_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(ws.parent, ws.acc, n, min_voxels, ws.counts, ws.partials);
    OAI_CHECK_LAUNCH();
    cc_finish_kernel<<<1, kT, 0, st>>>(ws.parent, ws.counts, ws.partials, ws.blocks, n, ws.nonfinite, ws.offsets, summary_dev);
    OAI_CHECK_LAUNCH();
    if (labels_dev) {
        cc_rank_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(ws.parent, ws.offsets, n, labels_dev);
        OAI_CHECK_LAUNCH();
    }
    if (labels_dev || size_dev) {
        cc_gather_kernel<<<per_voxel, kT, 0, st>>>(ws.parent, ws.acc, n, labels_dev, size_dev);
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

int oai_component_sizes(const int* labels_dev, long long n, long long n_components, long long* sizes_dev, void* stream) {
    OAI_CHECK_ARG(n >= 0 && n_components >= 0, "oai_component_sizes: negative count (n = %lld, n_components = %lld)", n, n_components);
    OAI_CHECK_ARG(n_components <= kMaxVoxels, "oai_component_sizes: labels are int32, n_components = %lld is not", n_components);
    if (n == 0 || n_components == 0) return OAI_OK;
    OAI_CHECK_ARG(labels_dev && sizes_dev, "oai_component_sizes: null pointer");
    OAI_CHECK_ARG(cdiv(n, kT) == (n + kT - 1) / kT, "oai_component_sizes: n = %lld is too large", n);
    const hipStream_t st = (hipStream_t)stream;
    OAI_CHECK_HIP(hipMemsetAsync(sizes_dev, 0, (size_t)n_components * sizeof(long long), st));
    cc_sizes_kernel<<<cdiv(n, kT), kT, 0, st>>>(labels_dev, n, n_components, (unsigned long long*)sizes_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
