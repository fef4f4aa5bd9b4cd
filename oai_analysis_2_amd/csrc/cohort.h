// What the cohort statistics sources share (csrc/group_stats.hip, group_regression.hip, graph_tfce.hip, graph_smooth.hip, cohort_pca.hip): the limits of
// their entry points and the argument checks of the graph ones, stated once, and the counted mean that both prepare kernels start with.
#pragma once
#include "common.h"

namespace oai {

constexpr long long kMaxKnees = 1LL << 24;
constexpr long long kMaxRows = 1LL << 20;          // of one batch or call
constexpr long long kMaxVerts = (1LL << 31) - 2;
constexpr int kDotChunk = 512;                     // vertices per chunk of the ordered dot (csrc/cohort_pca.hip): part of its stated order

// a cohort matrix [N][V], and a tile [rows][V] of per-row values on its vertices
static inline bool cohort_shape_ok(long long N, long long V) { return N >= 2 && N <= kMaxKnees && V >= 1 && V <= kMaxVerts; }
static inline bool tile_shape_ok(long long rows, long long V) { return rows >= 1 && rows <= kMaxRows && V >= 1 && V <= kMaxVerts; }

// The counted mean of vertex v over the knees of Y [N][V] that have a value there (mask null: all): n of them, summed in ascending knee
// index with one accumulator; mean = sum / n (NaN for n = 0).  No product: there is nothing here to contract.
struct CountedMean {
    int n;
    double mean;
};

__device__ __forceinline__ CountedMean counted_mean(const float* __restrict__ Y, const unsigned char* __restrict__ mask, long long N, long long V,
                                                    long long v) {
    int n = 0;
    double sum = 0.0;
    for (long long i = 0; i < N; ++i) {
        const bool m = mask ? mask[i * V + v] != 0 : true;
        n += m ? 1 : 0;
        sum = sum + (m ? (double)Y[i * V + v] : 0.0);
    }
    return {n, sum / (double)n};
}

// The checks of rows, vertices and neighbour count that every graph entry point (oai_graph_clusters, oai_graph_tfce, oai_graph_smooth)
// opens with; `who` is its name as a string literal, so every message keeps its text.
#define OAI_CHECK_GRAPH_TILE(who, n_rows, n_verts, n_neighbours)                                                                \
    do {                                                                                                                         \
        OAI_CHECK_ARG((n_rows) >= 1 && (n_rows) <= ::oai::kMaxRows, who ": needs 1 .. 2^20 rows (got %lld)", n_rows);            \
        OAI_CHECK_ARG((n_verts) >= 1 && (n_verts) <= ::oai::kMaxVerts, who ": needs 1 .. 2^31-2 vertices (got %lld)", n_verts);  \
        OAI_CHECK_ARG((n_neighbours) >= 0, who ": negative neighbour count (%lld)", n_neighbours);                               \
    } while (0)

}  // namespace oai
