// Rank transform for gfx950 (include/oai_hip.h, "Rank transform"; tests/rank_transform_ref.py restates this file a different way, through
// scipy.stats.rankdata): per vertex the midranks of the knees that have a value there, the rank sums of groups of knees, and scores of
// the ranks -- what Mann-Whitney, Wilcoxon signed-rank, Kruskal-Wallis, Spearman and the rank-based inverse-normal transform start from.
//   oai_column_ranks   values [N][V] (and a mask) -> twice the midrank per entry, the valid count and the tie term per vertex
//   oai_rank_sums      twice_rank [N][V], a group per knee (or the sign of the entry) -> per group and vertex the count and twice the rank sum
//   oai_rank_scores    twice_rank [N][V], n_valid [V] -> the rank, the centred rank or the normal score, float64, and the mask
//
// Ranks are COUNTS: twice_rank = 2 #{k_j < k_i} + #{k_j == k_i} + 1 over the valid j of the vertex.  Every output of the first two entry
// points is an integer formed by integer adds, so nothing depends on the launch geometry or on the order anything ran in; the one
// atomic is a 64-bit INTEGER add.  No floating-point atomics.
//
// Shape of the rank kernel.  A lane owns one vertex and kOwn of its rows, whose keys it holds in VGPRs; a wave64 covers 64 consecutive
// vertices, so that row j of the wave is one coalesced 256-byte load; the four waves of a 256-thread block own four CONSECUTIVE row
// groups of the SAME 64 vertices, so that the panel [N][64] they all walk is fetched from L2 once per block and three times from the
// CU's L1.  The inner loop walks all N rows once: per (own row, row j) two compares and two integer adds.  A row j that is not valid is
// given the key NaN, which neither `<` nor `==` admits: it is folded in by the compare itself and costs no branch; an own row that is not
// valid has the key NaN too and counts nothing.  Every wave counts the valid rows as it walks; the wave of row group 0 writes n_valid.
// tie_term takes one 64-bit integer atomicAdd per (row group, vertex) onto a vector zeroed by a launch before.
//   The schedule.  Per pair the ISA is v_cmp_lt, v_addc_co (the carry-in is the add), v_cmp_eq, v_addc_co: four vector instructions.
//   Left alone, the scheduler hoists all 32 compares of a row j above their adds and spills the 32 lane masks into vector lanes
//   (92 .. 127 VGPRs); a sched_barrier after every own row keeps a compare next to its add.  The next row's value and mask byte are
//   loaded BEFORE the compares of the current row and turned into a key after them, so the load is in flight under 64 instructions.
//   kOwn = 16: 16 keys + 32 counters.  The compiler's kernel-resource remarks on the gfx950 build with __launch_bounds__(256, 8), all
//   four instances: 64 VGPRs, 8 waves per SIMD, 108 .. 140 bytes of scratch per lane that the prologue and the epilogue touch once per
//   wave -- the loop over j holds no scratch instruction (profiles/rank_transform.md has the figures per instance and the timings: 41 ..
//   44 % of the VALU issue rate at N = 2000).  kOwn = 32 would halve the loads per compare and leave 4 waves per SIMD; it was not built.
// The form is O(N^2 V).  A sort-based form is not built; profiles/rank_transform.md says from which N it would pay.
//
// The normal score is Phi^-1 by Halley's iteration on the lower tail (the header states it); the device erfc, exp and log are not
// numpy's, so that ONE output is held to a tolerance and not to the bit.  fp64 without contraction.
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kOwn = 16;                           // own rows per lane
constexpr long long kMaxRankKnees = 1LL << 22;     // a midrank (a multiple of 1/2 up to N) is exact in float32
constexpr int kMaxGroups = 16;
constexpr int kLabelChunk = 1024;                  // labels per launch of sums_kernel: they travel as a kernel argument
constexpr int kHalley = 4;                         // the smallest count at which |device - scipy.special.ndtri| no longer improves

static inline bool rank_shape_ok(long long N, long long V) { return N >= 1 && N <= kMaxRankKnees && V >= 1 && V <= kMaxVerts; }

// ---- oai_column_ranks ------------------------------------------------------------------------------------------------------------------
template <bool SIGNED>
__device__ __forceinline__ float key_of(float y, unsigned char m) {
    bool ok = m != 0;
    if (SIGNED) ok = ok && y != 0.0f;
    return ok ? (SIGNED ? fabsf(y) : y) : NAN;       // a NaN value stays NaN: not valid either way
}

template <bool SIGNED, bool MASKED>
__device__ __forceinline__ float key_at(const float* __restrict__ Y, const unsigned char* __restrict__ mask, long long at) {
    return key_of<SIGNED>(Y[at], MASKED ? mask[at] : (unsigned char)1);
}

__global__ void __launch_bounds__(kT) zero_kernel(long long* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i < n) p[i] = 0;
}

// Block b is row-group quad b % quads of the 64-vertex block b / quads; its wave w owns rows [(4 (b % quads) + w) kOwn, + kOwn).  A lane
// past V works on vertex V - 1 and stores nothing; an own row past N has the key NaN.
template <bool SIGNED, bool MASKED>
__global__ void __launch_bounds__(kT, 8) ranks_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, long long N, long long V,
                                                   unsigned quads, int* __restrict__ twice_rank, int* __restrict__ n_valid,
                                                   long long* __restrict__ tie_term) {
    const long long v = (long long)(blockIdx.x / quads) * 64 + (threadIdx.x & 63);
    const long long vc = v < V ? v : V - 1;
    const long long group = (long long)(blockIdx.x % quads) * kWaves + (threadIdx.x >> 6);
    const long long i0 = group * kOwn;
    if (i0 >= N) return;                                                  // uniform over the wave; no barrier follows
    float key[kOwn];
    int less[kOwn], equal[kOwn];
#pragma unroll
    for (int r = 0; r < kOwn; ++r) {
        key[r] = i0 + r < N ? key_at<SIGNED, MASKED>(Y, mask, (i0 + r) * V + vc) : NAN;
        less[r] = 0;
        equal[r] = 0;
    }
    int n = 0;
    float kj = key_at<SIGNED, MASKED>(Y, mask, vc);
#pragma unroll 1
    for (long long j = 0; j < N; ++j) {
        const long long at = (j + 1 < N ? j + 1 : j) * V + vc;             // the next row's loads are in flight under this row's compares
        const float y_next = Y[at];
        const unsigned char m_next = MASKED ? mask[at] : (unsigned char)1;
        __builtin_amdgcn_sched_barrier(0);
        n += kj == kj ? 1 : 0;
#pragma unroll
        for (int r = 0; r < kOwn; ++r) {
            less[r] += kj < key[r] ? 1 : 0;
            equal[r] += kj == key[r] ? 1 : 0;
            __builtin_amdgcn_sched_barrier(0);                            // a compare, then its add: see the note on the schedule above
        }
        kj = key_of<SIGNED>(y_next, m_next);
    }
    if (v >= V) return;
    long long ties = 0;
#pragma unroll
    for (int r = 0; r < kOwn; ++r) {
        if (i0 + r >= N) continue;
        const bool ok = key[r] == key[r];
        int tr = ok ? 2 * less[r] + equal[r] + 1 : 0;
        if (SIGNED && ok && Y[(i0 + r) * V + v] < 0.0f) tr = -tr;
        twice_rank[(i0 + r) * V + v] = tr;
        ties += ok ? (long long)equal[r] * (long long)equal[r] - 1 : 0;
    }
    if (group == 0) n_valid[v] = n;
    if (ties != 0) atomicAdd((unsigned long long*)(tie_term + v), (unsigned long long)ties);
}

template <bool SIGNED, bool MASKED>
int launch_ranks(const float* Y, const unsigned char* mask, long long N, long long V, int* twice_rank, int* n_valid, long long* tie_term,
                 hipStream_t st) {
    const unsigned quads = cdiv(N, (long long)kOwn * kWaves);
    const long long blocks = (long long)cdiv(V, 64) * quads;
    OAI_CHECK_ARG(blocks < (1LL << 31), "oai_column_ranks: n_knees = %lld and n_verts = %lld are more than one launch takes: rank a shorter span of vertices", N,
                  V);
    zero_kernel<<<cdiv(V, kT), kT, 0, st>>>(tie_term, V);
    OAI_CHECK_LAUNCH();
    ranks_kernel<SIGNED, MASKED><<<(unsigned)blocks, kT, 0, st>>>(Y, mask, N, V, quads, twice_rank, n_valid, tie_term);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// ---- oai_rank_sums ---------------------------------------------------------------------------------------------------------------------
struct Labels {
    unsigned char g[kLabelChunk];
};

// One thread per (vertex, group g = blockIdx.y), rows [i0, i0 + rows) ascending; the label of a row is wave-uniform and comes from the
// kernel argument.  BY_SIGN: group 0 the negative entries, group 1 the positive ones.  The first chunk writes, a later one adds to what
// the chunk before it wrote (launches of one stream run in order; each element has one owner): integer sums, exact in any order.
template <bool BY_SIGN>
__global__ void __launch_bounds__(kT) sums_kernel(const int* __restrict__ twice_rank, Labels labels, long long i0, int rows, long long V, int first,
                                                  int* __restrict__ n_g, long long* __restrict__ twice_sum_g) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    const int g = blockIdx.y;
    int n = 0;
    long long sum = 0;
    for (int r = 0; r < rows; ++r) {
        const int tr = twice_rank[(i0 + r) * V + v];
        const bool in = BY_SIGN ? (g == 0 ? tr < 0 : tr > 0) : (tr != 0 && labels.g[r] == g);
        n += in ? 1 : 0;
        sum += in ? (long long)(tr < 0 ? -tr : tr) : 0;
    }
    const long long at = (long long)g * V + v;
    n_g[at] = first ? n : n_g[at] + n;
    twice_sum_g[at] = first ? sum : twice_sum_g[at] + sum;
}

// ---- oai_rank_scores -------------------------------------------------------------------------------------------------------------------
// Phi^-1(p), 0 < p < 1, as the header states it
__device__ __forceinline__ double inverse_normal(double p) {
    const double q = p < 1.0 - p ? p : 1.0 - p;
    double x = q > 0.2 ? 2.5 * (q - 0.5) : -sqrt(-2.0 * log(q));
#pragma unroll 1
    for (int k = 0; k < kHalley; ++k) {
        const double F = 0.5 * erfc(-x * 0.70710678118654752440);
        const double phi = exp(-0.5 * x * x) * 0.39894228040143267794;
        const double u = (F - q) / phi;
        x = x - u / (1.0 + 0.5 * x * u);
    }
    return p > 0.5 ? -x : x;
}

template <int KIND>
__global__ void __launch_bounds__(kT) scores_kernel(const int* __restrict__ twice_rank, const int* __restrict__ n_valid, long long total, long long V,
                                                    double c, double* __restrict__ score, unsigned char* __restrict__ mask) {
    for (long long at = (long long)blockIdx.x * kT + threadIdx.x; at < total; at += (long long)gridDim.x * kT) {
        const int tr = twice_rank[at];
        const double n = (double)n_valid[at % V];
        double s = 0.0;
        if (tr != 0) {
            if (KIND == OAI_SCORE_RANK) s = 0.5 * (double)tr;
            if (KIND == OAI_SCORE_CENTRED) s = 0.5 * (double)tr - 0.5 * (n + 1.0);
            if (KIND == OAI_SCORE_NORMAL) {
                const double r = 0.5 * (double)(tr < 0 ? -tr : tr);
                const double x = inverse_normal((r - c) / ((n - 2.0 * c) + 1.0));
                s = tr < 0 ? -x : x;
            }
        }
        score[at] = s;
        mask[at] = tr != 0 ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int oai_column_ranks(const float* values_dev, const unsigned char* mask_dev, long long n_knees, long long n_verts, int mode, int* twice_rank_dev,
                     int* n_valid_dev, long long* tie_term_dev, void* stream) {
    OAI_CHECK_ARG(rank_shape_ok(n_knees, n_verts), "oai_column_ranks: needs n_knees 1 .. 2^22 and n_verts 1 .. 2^31-2 (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(mode == OAI_RANK_PLAIN || mode == OAI_RANK_SIGNED, "oai_column_ranks: mode must be OAI_RANK_PLAIN (0) or OAI_RANK_SIGNED (1), got %d", mode);
    OAI_CHECK_ARG(values_dev, "oai_column_ranks: values_dev is a null pointer");
    OAI_CHECK_ARG(twice_rank_dev && n_valid_dev && tie_term_dev, "oai_column_ranks: null pointer among twice_rank_dev, n_valid_dev, tie_term_dev");
    const hipStream_t st = (hipStream_t)stream;
    if (mode == OAI_RANK_SIGNED)
        return mask_dev ? launch_ranks<true, true>(values_dev, mask_dev, n_knees, n_verts, twice_rank_dev, n_valid_dev, tie_term_dev, st)
                        : launch_ranks<true, false>(values_dev, nullptr, n_knees, n_verts, twice_rank_dev, n_valid_dev, tie_term_dev, st);
    return mask_dev ? launch_ranks<false, true>(values_dev, mask_dev, n_knees, n_verts, twice_rank_dev, n_valid_dev, tie_term_dev, st)
                    : launch_ranks<false, false>(values_dev, nullptr, n_knees, n_verts, twice_rank_dev, n_valid_dev, tie_term_dev, st);
}

int oai_rank_sums(const int* twice_rank_dev, const unsigned char* labels_host, long long n_knees, long long n_verts, int n_groups, int* n_g_dev,
                  long long* twice_sum_g_dev, void* stream) {
    OAI_CHECK_ARG(rank_shape_ok(n_knees, n_verts), "oai_rank_sums: needs n_knees 1 .. 2^22 and n_verts 1 .. 2^31-2 (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(n_groups >= 1 && n_groups <= kMaxGroups, "oai_rank_sums: n_groups must be 1 .. 16, got %d", n_groups);
    OAI_CHECK_ARG(labels_host || n_groups == 2, "oai_rank_sums: null labels_host groups by sign and needs n_groups = 2, got %d", n_groups);
    OAI_CHECK_ARG(twice_rank_dev, "oai_rank_sums: twice_rank_dev is a null pointer");
    OAI_CHECK_ARG(n_g_dev && twice_sum_g_dev, "oai_rank_sums: null pointer among n_g_dev, twice_sum_g_dev");
    if (labels_host)
        for (long long i = 0; i < n_knees; ++i)
            OAI_CHECK_ARG(labels_host[i] < n_groups, "oai_rank_sums: labels_host[%lld] = %d is not below n_groups = %d", i, (int)labels_host[i], n_groups);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(n_verts, kT), (unsigned)n_groups);
    Labels labels = {};
    for (long long i0 = 0; i0 < n_knees; i0 += kLabelChunk) {
        const int rows = (int)(n_knees - i0 < kLabelChunk ? n_knees - i0 : kLabelChunk);
        if (labels_host) {
            for (int r = 0; r < rows; ++r) labels.g[r] = labels_host[i0 + r];
            sums_kernel<false><<<grid, kT, 0, st>>>(twice_rank_dev, labels, i0, rows, n_verts, i0 == 0 ? 1 : 0, n_g_dev, twice_sum_g_dev);
        } else {
            sums_kernel<true><<<grid, kT, 0, st>>>(twice_rank_dev, labels, i0, rows, n_verts, i0 == 0 ? 1 : 0, n_g_dev, twice_sum_g_dev);
        }
        OAI_CHECK_LAUNCH();
    }
    return OAI_OK;
}

int oai_rank_scores(const int* twice_rank_dev, const int* n_valid_dev, long long n_knees, long long n_verts, int kind, double c, double* score_dev,
                    unsigned char* mask_dev, void* stream) {
    OAI_CHECK_ARG(rank_shape_ok(n_knees, n_verts), "oai_rank_scores: needs n_knees 1 .. 2^22 and n_verts 1 .. 2^31-2 (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(kind == OAI_SCORE_RANK || kind == OAI_SCORE_CENTRED || kind == OAI_SCORE_NORMAL,
                  "oai_rank_scores: kind must be OAI_SCORE_RANK (0), OAI_SCORE_CENTRED (1) or OAI_SCORE_NORMAL (2), got %d", kind);
    OAI_CHECK_ARG(c >= 0.0 && c <= 0.5, "oai_rank_scores: c must lie in [0, 1/2], got %g", c);
    OAI_CHECK_ARG(twice_rank_dev && n_valid_dev, "oai_rank_scores: null pointer among twice_rank_dev, n_valid_dev");
    OAI_CHECK_ARG(score_dev && mask_dev, "oai_rank_scores: null pointer among score_dev, mask_dev");
    const hipStream_t st = (hipStream_t)stream;
    const long long total = n_knees * n_verts;
    const unsigned blocks = grid_stride_blocks(total, kT);
    if (kind == OAI_SCORE_RANK) scores_kernel<OAI_SCORE_RANK><<<blocks, kT, 0, st>>>(twice_rank_dev, n_valid_dev, total, n_verts, c, score_dev, mask_dev);
    if (kind == OAI_SCORE_CENTRED) scores_kernel<OAI_SCORE_CENTRED><<<blocks, kT, 0, st>>>(twice_rank_dev, n_valid_dev, total, n_verts, c, score_dev, mask_dev);
    if (kind == OAI_SCORE_NORMAL) scores_kernel<OAI_SCORE_NORMAL><<<blocks, kT, 0, st>>>(twice_rank_dev, n_valid_dev, total, n_verts, c, score_dev, mask_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
