// Longitudinal change for gfx950 (include/oai_hip.h, "Longitudinal change"; tests/visit_slopes_ref.py restates this file operation for
// operation): stage one of the two-stage (summary-measures) analysis.  Every subject has a run of visits -- rows of the visit matrix with a
// time in years -- and per (subject, vertex) a straight line is fitted through the visits that have a value at that vertex:
//   oai_visit_slopes     the slot table into the workspace (one small launch), then one launch that writes, per (subject, vertex), the
//                        count n, the slope (rate), the mean (avg), the fitted value at the subject's reference time (fit_ref), the
//                        residual standard deviation (resid_sd) and ok as a mask
//
// fp64 without contraction; the order IS the contract, as in csrc/group_stats.hip: three passes over the subject's slots in ascending CSR
// position, one accumulator per sum in one thread, sums centred on the means of pass 1.  A slot that is missing at the vertex is
// skipped by a select, never multiplied by 0.  No atomics of any kind; every output element is formed by one thread from the inputs
// alone, so the bits do not depend on the launch geometry.
//
// Shape, and why.  A thread owns one (subject, vertex) with the vertex fastest: a wave64 reads 64 consecutive floats (256 bytes) and 64
// mask bytes of a visit row per slot, and writes runs of 512 bytes.  The subject is blockIdx.y (strided by gridDim.y beyond 65 535
// subjects), so the slot run [a, b), the row and the time of a slot are the same in every lane of a block: they are read through scalar
// loads, and every branch on them is uniform.
//   slot_table_kernel writes what the hot kernel would otherwise re-derive per thread and slot: per subject the slot run with its
//     offsets clamped into [0, n_visits] (int2), per slot the row, or -1 for a row outside [0, n_rows).  That is the workspace.
//   A slot of row -1 reads row 0 (which always exists) and is dropped by the select: the loads are unconditional, so that the loads
//     of a pass can all be in flight together.
//   The three passes need every (value, mask byte) three times.  The first kHold = 8 slots of a subject are loaded ONCE, all in flight
//     together, and held in registers (8 floats and one word of mask bits); a slot beyond them is re-read in every pass from the
//     subject's rows, which the first pass has just brought into L2.  An OAI study has at most ten visits and most knees fewer than
//     eight, so the re-read is the tail case; a run of 40 visits takes 8 slots from registers and 32 by re-reading.  Both routes
//     apply the same operations to the same numbers in the same order: the same bits.  kHold = 0 (every slot re-read in every pass) is
//     the other design; it exists in diagnostic builds only (OAI_VISIT_SLOPES_HOLD=0) and lost by a fifth: 0.32 ms against 0.25 ms
//     for the call on 200 subjects x 7 visits x 30 002 vertices (49 VGPRs and 7 waves per SIMD against 28 and 8, no scratch either way).
//   A null output is not written, and the pass that only it needs does not run: pass 3 runs for resid_sd alone, pass 2 for everything
//     but n.
// Measured (profiles/longitudinal.md): that shape with all six outputs, 194 us in the kernel -- 2.2 TB/s of the 432 MB it must move, 2.8
// times the copy floor, 11 times faster than the same sums as torch ops.  The loads are 4 and 1 bytes per lane; rows of 30 002 floats do not
// start on 16 bytes, so wider loads would need a peeled head per row and were not tried.
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kSlopesT = 256;                      // vertices of a block
constexpr int kHold = 8;                           // slots of a subject held in registers over the three passes
constexpr unsigned kMaxGridY = 65535;

struct SlopesWs {
    int2* run;                                     // [n_subjects]: the slots [x, y) of the subject, inside [0, n_visits]
    int* row;                                      // [n_visits]: the row of the slot, -1 when it names none
    size_t bytes;
    SlopesWs(const void* base, long long n_subjects, long long n_visits) {
        Ws ws(base);
        run = ws.take<int2>((size_t)n_subjects);
        row = ws.take<int>((size_t)n_visits);
        bytes = ws.off;
    }
};

static inline bool slopes_shape_ok(long long n_rows, long long n_verts, long long n_subjects, long long n_visits) {
    return n_rows >= 1 && n_rows <= kMaxKnees && n_verts >= 1 && n_verts <= kMaxVerts && n_subjects >= 1 && n_subjects <= kMaxKnees &&
           n_visits >= 0 && n_visits <= kMaxKnees;
}

struct SlopesOut {
    double *rate, *avg, *fit_ref, *resid_sd;
    int* n;
    unsigned char* mask;
};

__global__ void __launch_bounds__(kSlopesT) slot_table_kernel(const int* __restrict__ offsets, const int* __restrict__ visit_row, int n_rows,
                                                              int n_subjects, int n_visits, int2* __restrict__ run, int* __restrict__ row) {
    const int i = blockIdx.x * kSlopesT + threadIdx.x;
    if (i < n_subjects) {
        int a = offsets[i], b = offsets[i + 1];
        a = a < 0 ? 0 : (a > n_visits ? n_visits : a);
        b = b < 0 ? 0 : (b > n_visits ? n_visits : b);
        run[i] = make_int2(a, b);
    }
    if (i < n_visits) {
        const int r = visit_row[i];
        row[i] = (r >= 0 && r < n_rows) ? r : -1;
    }
}

struct Visit {
    bool m;
    float y;
};

// slot e at vertex v: the loads are unconditional (a slot without a row reads row 0), what they bring is dropped by the caller's select
__device__ __forceinline__ Visit load_visit(const float* __restrict__ values, const unsigned char* __restrict__ mask, const int* __restrict__ row, int e,
                                            long long V, long long v) {
    const int r = row[e];
    const long long at = (long long)(r >= 0 ? r : 0) * V + v;
    const bool m = (r >= 0) & (mask ? mask[at] != 0 : true);
    return {m, values[at]};
}

template <int HOLD>
__global__ void __launch_bounds__(kSlopesT) visit_slopes_kernel(const float* __restrict__ values, const unsigned char* __restrict__ mask, long long V,
                                                                const int2* __restrict__ run, const int* __restrict__ row,
                                                                const double* __restrict__ time, const double* __restrict__ reference_time,
                                                                int n_subjects, int min_visits, double min_span, SlopesOut out) {
    const long long v = (long long)blockIdx.x * kSlopesT + threadIdx.x;
    if (v >= V) return;
    const bool fit = out.rate || out.avg || out.fit_ref || out.resid_sd || out.mask;
    for (int s = blockIdx.y; s < n_subjects; s += gridDim.y) {
        const int2 ab = run[s];
        const int a = ab.x, b = ab.y;
        // the first HOLD slots: loaded once, together
        float held_y[HOLD > 0 ? HOLD : 1];
        unsigned held_m = 0;
#pragma unroll
        for (int k = 0; k < HOLD; ++k) {
            held_y[k] = 0.0f;
            if (a + k < b) {                                               // uniform over the block
                const Visit w = load_visit(values, mask, row, a + k, V, v);
                held_y[k] = w.y;
                held_m |= (w.m ? 1u : 0u) << k;
            }
        }
        // f(t_e, valid at v, y_e) for every slot of the subject in ascending CSR position
        auto each_slot = [&](auto&& f) {
#pragma unroll
            for (int k = 0; k < HOLD; ++k)
                if (a + k < b) f(time[a + k], ((held_m >> k) & 1u) != 0, (double)held_y[k]);
            for (int e = a + HOLD; e < b; ++e) {
                const Visit w = load_visit(values, mask, row, e, V, v);
                f(time[e], w.m, (double)w.y);
            }
        };

        // pass 1
        int n = 0;
        double St = 0.0, Sy = 0.0, tmin = INFINITY, tmax = -INFINITY;
        each_slot([&](double t, bool m, double y) {
            const double st = St + t, sy = Sy + y;
            n += m ? 1 : 0;
            St = m ? st : St;                                              // a select: what lies under a 0 mask byte reaches no sum
            Sy = m ? sy : Sy;
            tmin = (m && t < tmin) ? t : tmin;
            tmax = (m && t > tmax) ? t : tmax;
        });
        const long long at = (long long)s * V + v;
        if (out.n) out.n[at] = n;
        if (!fit) continue;
        const double tb = St / (double)n, yb = Sy / (double)n;             // n = 0: NaN, and ok is false

        // pass 2
        double Sxx = 0.0, Sxy = 0.0;
        each_slot([&](double t, bool m, double y) {
            const double dt = t - tb, dy = y - yb;
            const double pxx = dt * dt, pxy = dt * dy;
            const double sxx = Sxx + pxx, sxy = Sxy + pxy;
            Sxx = m ? sxx : Sxx;
            Sxy = m ? sxy : Sxy;
        });
        const bool ok = n >= min_visits && Sxx > 0.0 && (tmax - tmin) >= min_span;
        const double rate = Sxy / Sxx;
        if (out.mask) out.mask[at] = ok ? 1 : 0;
        if (out.rate) out.rate[at] = ok ? rate : 0.0;
        if (out.avg) out.avg[at] = ok ? yb : 0.0;
        if (out.fit_ref) {
            const double ahead = reference_time[s] - tb, p = rate * ahead;
            out.fit_ref[at] = ok ? yb + p : 0.0;
        }
        if (!out.resid_sd) continue;

        // pass 3
        double rss = 0.0;
        each_slot([&](double t, bool m, double y) {
            const double dt = t - tb, dy = y - yb;
            const double p = rate * dt, r = dy - p, rr = r * r;
            const double next = rss + rr;
            rss = m ? next : rss;
        });
        out.resid_sd[at] = ok ? (n >= 3 ? sqrt(rss / (double)(n - 2)) : (double)NAN) : 0.0;
    }
}

}  // namespace

extern "C" {

size_t oai_visit_slopes_workspace_bytes(long long n_rows, long long n_verts, long long n_subjects, long long n_visits) {
    if (!slopes_shape_ok(n_rows, n_verts, n_subjects, n_visits)) return 0;
    return SlopesWs(nullptr, n_subjects, n_visits).bytes;
}

int oai_visit_slopes(const float* values_dev, const unsigned char* mask_dev, long long n_rows, long long n_verts, const int* subject_offsets_dev,
                     long long n_subjects, const int* visit_row_dev, const double* visit_time_dev, long long n_visits,
                     const double* reference_time_dev, int min_visits, double min_span, void* workspace_dev, size_t workspace_bytes,
                     double* rate_dev, double* avg_dev, double* fit_ref_dev, double* resid_sd_dev, int* n_dev, unsigned char* out_mask_dev,
                     void* stream) {
    OAI_CHECK_ARG(n_rows >= 1 && n_rows <= kMaxKnees, "oai_visit_slopes: needs 1 .. 2^24 rows (n_rows), got %lld", n_rows);
    OAI_CHECK_ARG(n_verts >= 1 && n_verts <= kMaxVerts, "oai_visit_slopes: needs 1 .. 2^31-2 vertices (n_verts), got %lld", n_verts);
    OAI_CHECK_ARG(n_subjects >= 1 && n_subjects <= kMaxKnees, "oai_visit_slopes: needs 1 .. 2^24 subjects (n_subjects), got %lld", n_subjects);
    OAI_CHECK_ARG(n_visits >= 0 && n_visits <= kMaxKnees, "oai_visit_slopes: needs 0 .. 2^24 visits (n_visits), got %lld", n_visits);
    OAI_CHECK_ARG(min_visits >= 2, "oai_visit_slopes: min_visits must be at least 2, got %d", min_visits);
    OAI_CHECK_ARG(min_span >= 0.0 && std::isfinite(min_span), "oai_visit_slopes: min_span must be finite and >= 0, got %g", min_span);
    OAI_CHECK_ARG(values_dev && subject_offsets_dev && reference_time_dev && workspace_dev && (n_visits == 0 || (visit_row_dev && visit_time_dev)),
                  "oai_visit_slopes: null pointer");
    OAI_CHECK_WORKSPACE("oai_visit_slopes", workspace_bytes, oai_visit_slopes_workspace_bytes(n_rows, n_verts, n_subjects, n_visits));
    const SlopesWs ws(workspace_dev, n_subjects, n_visits);
    hipStream_t st = (hipStream_t)stream;
    const long long entries = n_subjects > n_visits ? n_subjects : n_visits;
    slot_table_kernel<<<cdiv(entries, kSlopesT), kSlopesT, 0, st>>>(subject_offsets_dev, visit_row_dev, (int)n_rows, (int)n_subjects, (int)n_visits, ws.run,
                                                                   ws.row);
    OAI_CHECK_LAUNCH();
    const SlopesOut out{rate_dev, avg_dev, fit_ref_dev, resid_sd_dev, n_dev, out_mask_dev};
    if (!(rate_dev || avg_dev || fit_ref_dev || resid_sd_dev || n_dev || out_mask_dev)) return OAI_OK;
    const dim3 grid(cdiv(n_verts, kSlopesT), n_subjects < (long long)kMaxGridY ? (unsigned)n_subjects : kMaxGridY);
#ifdef OAI_DIAG
    if (diag_env("OAI_VISIT_SLOPES_HOLD", kHold) == 0) {                  // the design that lost: every slot re-read in every pass
        visit_slopes_kernel<0><<<grid, kSlopesT, 0, st>>>(values_dev, mask_dev, n_verts, ws.run, ws.row, visit_time_dev, reference_time_dev,
                                                         (int)n_subjects, min_visits, min_span, out);
        OAI_CHECK_LAUNCH();
        return OAI_OK;
    }
#endif
    visit_slopes_kernel<kHold><<<grid, kSlopesT, 0, st>>>(values_dev, mask_dev, n_verts, ws.run, ws.row, visit_time_dev, reference_time_dev,
                                                         (int)n_subjects, min_visits, min_span, out);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
