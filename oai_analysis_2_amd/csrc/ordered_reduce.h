// The ordered block reduction of the QC kernels (csrc/phi_jacobian.hip, csrc/phi_inverse.hip, csrc/edt.hip).  Device code only.
//
// The order IS the contract: include/oai_hip.h promises bit-reproducible fp64 statistics, and tests/ordered_reduce_ref.py restates this
// file operation for operation (tests/test_edt_gpu.py pins the device to it).  An accumulator type provides
//   T v[N];   void clear();   void merge(const T* o);      merge: this (the earlier elements) on the left of every operation
// and a reduction is
//   1. per thread, the caller's own loop in its own order;
//   2. block_reduce: inside each wave64, for off = 32, 16, ..., 1: v[lane] = merge(v[lane], v[lane + off]) through __shfl_down (a lane
//      whose partner is past the wave reads its own value; such a lane never reaches lane 0); lane 0 of each wave to lds[wave]; a block
//      barrier; thread 0 merges waves 1, 2, ... in order.  Valid in thread 0 only;
//   3. one slot of N values per block in the workspace, then a one-block finish kernel: reduce_slots (thread t merges its run of
//      consecutive slots in index order into a cleared accumulator), then block_reduce again.
// No atomics, and the number of slots depends on the shape only.
//
// NOT users, on purpose: block_sum / block_min / block_excl_scan / mm_block_store (csrc/mesh_split.hip), block_sum_store /
// block_ext_store (csrc/thickness_map.hip), block_reduce of csrc/mesh_graph.hip and the scan of csrc/mesh.hip.  They are other trees
// (__shfl_xor butterflies, LDS halving over 256 threads), their fp64 sums feed the k-means and the circle fits, and moving them onto
// this tree would change those bits.
#pragma once
#include <hip/hip_runtime.h>

namespace oai {

template <int kT, class Acc, class T, int N>
__device__ __forceinline__ void block_reduce(Acc& a, T (*lds)[N]) {
    static_assert(kT % 64 == 0 && sizeof(a.v) == sizeof(T) * N, "whole waves, and one LDS row per accumulator");
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        T o[N];
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = __shfl_down(a.v[i], off, 64);
        a.merge(o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < N; ++i) lds[wave][i] = a.v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kT / 64; ++w) a.merge(lds[w]);
}

// thread t of a kT-thread block: slots [t per, min((t + 1) per, nb)) of `partials` in index order, per = ceil(nb / kT)
template <int kT, class Acc, class T>
__device__ __forceinline__ void reduce_slots(const T* __restrict__ partials, long long nb, Acc& acc) {
    constexpr int N = (int)(sizeof(acc.v) / sizeof(T));
    const long long per = (nb + kT - 1) / kT;
    const long long i0 = min(per * (long long)threadIdx.x, nb), i1 = min(i0 + per, nb);
    acc.clear();
    for (long long i = i0; i < i1; ++i) acc.merge(partials + i * N);
}

}  // namespace oai
