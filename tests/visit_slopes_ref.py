"""The numpy restatement of csrc/visit_slopes.hip (include/oai_hip.h, "Longitudinal change"): per (subject, vertex) a straight line through
the subject's visits that are valid at the vertex, in three passes over the subject's CSR slots in ascending position with one
accumulator per sum.  ``fit`` is vectorised over subjects and vertices and loops over the slot POSITION 0 .. longest run - 1, so that
every (subject, vertex) still adds its slots in ascending position; a slot that is skipped is skipped by np.where, never multiplied by 0.
``fit_loop`` is the header's rule written out as a plain Python loop, one float at a time: the two must agree to the bit.  numpy's
float64 add, multiply, divide and sqrt are IEEE and unfused, so the device must give the same bits.  ``measure`` restates the four
measures of ``LongitudinalCohort.change``; the generator of OAI-like visit schedules that the tests share is here as well."""
import math

import numpy as np

OUTPUTS = ("rate", "avg", "fit_ref", "resid_sd", "n", "mask")
OAI_VISIT_YEARS = (0.0, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0, 8.0)       # baseline and the follow-ups with MR imaging, nominal


def slot_runs(offsets, n_visits):
    """(lo, count) per subject: the offsets clamped into [0, n_visits] as the header says; an inverted run is empty."""
    off = np.asarray(offsets, np.int64).reshape(-1)
    lo, hi = np.clip(off[:-1], 0, n_visits), np.clip(off[1:], 0, n_visits)
    return lo, np.maximum(hi - lo, 0)


def fit(values, mask, offsets, rows, times, reference_time, min_visits=2, min_span=0.0):
    """dict of the six outputs, each [S, V]: rate, avg, fit_ref, resid_sd float64 (+0.0 where mask is 0), n int32, mask uint8."""
    Y = np.atleast_2d(np.asarray(values, np.float32))
    R, V = Y.shape
    M = np.ones((R, V), bool) if mask is None else np.atleast_2d(np.asarray(mask)) != 0
    rows, times = np.asarray(rows, np.int64).reshape(-1), np.asarray(times, np.float64).reshape(-1)
    tref = np.asarray(reference_time, np.float64).reshape(-1)
    lo, count = slot_runs(offsets, len(rows))
    S = len(lo)
    assert len(times) == len(rows) and len(tref) == S and min_visits >= 2 and min_span >= 0

    def slots():
        """(t [S, 1], valid [S, V], y float64 [S, V]) per slot position."""
        for k in range(int(count.max()) if S else 0):
            has = count > k
            e = np.where(has, lo + k, 0)
            r = rows[e] if len(rows) else np.zeros(S, np.int64)
            has = has & (r >= 0) & (r < R)
            r = np.where(has, r, 0)
            t = times[e] if len(times) else np.zeros(S)
            yield t[:, None], has[:, None] & M[r], Y[r].astype(np.float64)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = np.zeros((S, V), np.int32)
        St, Sy = np.zeros((S, V)), np.zeros((S, V))
        tmin, tmax = np.full((S, V), np.inf), np.full((S, V), -np.inf)
        for t, m, y in slots():
            n = n + m
            St, Sy = np.where(m, St + t, St), np.where(m, Sy + y, Sy)
            tmin, tmax = np.where(m & (t < tmin), t, tmin), np.where(m & (t > tmax), t, tmax)
        tb, yb = St / n, Sy / n
        Sxx, Sxy = np.zeros((S, V)), np.zeros((S, V))
        for t, m, y in slots():
            dt, dy = t - tb, y - yb
            Sxx, Sxy = np.where(m, Sxx + dt * dt, Sxx), np.where(m, Sxy + dt * dy, Sxy)
        ok = (n >= min_visits) & (Sxx > 0) & ((tmax - tmin) >= min_span)
        rate = Sxy / Sxx
        rss = np.zeros((S, V))
        for t, m, y in slots():
            dt, dy = t - tb, y - yb
            r = dy - rate * dt
            rss = np.where(m, rss + r * r, rss)
        fit_ref = yb + rate * (tref[:, None] - tb)
        resid_sd = np.where(n >= 3, np.sqrt(rss / np.where(n >= 3, n - 2, 1).astype(np.float64)), np.nan)
    zero = np.zeros((S, V))
    return {"rate": np.where(ok, rate, zero), "avg": np.where(ok, yb, zero), "fit_ref": np.where(ok, fit_ref, zero),
            "resid_sd": np.where(ok, resid_sd, zero), "n": n.astype(np.int32), "mask": ok.astype(np.uint8)}


def fit_loop(values, mask, offsets, rows, times, reference_time, min_visits=2, min_span=0.0):
    """The same by the header's rule, one Python float at a time."""
    Y = np.atleast_2d(np.asarray(values, np.float32))
    R, V = Y.shape
    E, S = len(rows), len(offsets) - 1
    out = {name: np.zeros((S, V), {"n": np.int32, "mask": np.uint8}.get(name, np.float64)) for name in OUTPUTS}
    for s in range(S):
        a, b = min(max(int(offsets[s]), 0), E), min(max(int(offsets[s + 1]), 0), E)
        for v in range(V):
            valid = [(float(times[e]), float(Y[int(rows[e]), v])) for e in range(a, b)
                     if 0 <= int(rows[e]) < R and (mask is None or mask[int(rows[e])][v] != 0)]
            n, St, Sy = len(valid), 0.0, 0.0
            out["n"][s, v] = n
            if n == 0:
                continue
            for t, y in valid:
                St, Sy = St + t, Sy + y
            tmin, tmax = min(t for t, _ in valid), max(t for t, _ in valid)
            tb, yb = St / n, Sy / n
            Sxx, Sxy = 0.0, 0.0
            for t, y in valid:
                dt, dy = t - tb, y - yb
                Sxx, Sxy = Sxx + dt * dt, Sxy + dt * dy
            if not (n >= min_visits and Sxx > 0 and (tmax - tmin) >= min_span):
                continue
            rate = Sxy / Sxx
            rss = 0.0
            for t, y in valid:
                dt, dy = t - tb, y - yb
                r = dy - rate * dt
                rss = rss + r * r
            out["mask"][s, v], out["rate"][s, v], out["avg"][s, v] = 1, rate, yb
            out["fit_ref"][s, v] = yb + rate * (float(reference_time[s]) - tb)
            out["resid_sd"][s, v] = math.sqrt(rss / float(n - 2)) if n >= 3 else math.nan
    return out


def measure(fitted, name):
    """(float32 [S, V] with 0 where missing, uint8 mask) of a measure of ``LongitudinalCohort.change``: "rate", "avg", or the rate in per
    cent of the fitted value at the reference time ("pc1") or of the mean ("spc") -- an IEEE divide, then a multiply by 100, in float64,
    missing where the denominator is not > 0 -- rounded to float32 once."""
    ok = fitted["mask"] != 0
    if name in ("rate", "avg"):
        x = fitted[name]
    else:
        den = fitted[{"pc1": "fit_ref", "spc": "avg"}[name]]
        ok = ok & (den > 0)
        x = (fitted["rate"] / np.where(ok, den, 1.0)) * 100.0
    return np.where(ok, x, 0.0).astype(np.float32), ok.astype(np.uint8)


# ---- visit schedules -------------------------------------------------------------------------------------------------------------------
def oai_like_schedule(rng, n_subjects, lo=2, hi=7, jitter=0.08):
    """Per subject ``lo`` .. ``hi`` of the nominal OAI visit years, drawn without replacement and jittered by up to +-``jitter`` years (a
    visit is booked within a window, not on the day), ascending: a list of float64 arrays."""
    out = []
    for _ in range(n_subjects):
        k = int(rng.integers(lo, hi + 1))
        years = np.sort(rng.choice(OAI_VISIT_YEARS, k, replace=False))
        out.append(years + rng.uniform(-jitter, jitter, k))
    return out


def oai_like_knees(seed, n_subjects, lo=2, hi=7):
    """One vertex per subject: (values float32 [R, 1], offsets, rows, times, reference_time) -- thickness of 1 to 4 mm at baseline, a loss
    of 0 to 0.1 mm a year and 0.05 mm of noise, one row per (subject, visit) in order."""
    rng = np.random.default_rng(seed)
    schedule = oai_like_schedule(rng, n_subjects, lo, hi)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in schedule])]).astype(np.int32)
    times = np.concatenate(schedule)
    base, loss = rng.uniform(1.0, 4.0, n_subjects), rng.uniform(0.0, 0.1, n_subjects)
    owner = np.repeat(np.arange(n_subjects), np.diff(offsets))
    y = np.clip(base[owner] - loss[owner] * times + rng.normal(0.0, 0.05, len(times)), 1.0, 4.0).astype(np.float32)
    return y[:, None], offsets, np.arange(len(times), dtype=np.int32), times, np.array([t[0] for t in schedule])


HOSTILE_COUNTS = (0, 1, 2, 40, 5)


def hostile_case(seed, V, counts=HOSTILE_COUNTS, with_mask=True):
    """(values, mask, offsets, rows, times, reference_time) of subjects with ``counts`` visits on a visit matrix with twelve rows more than
    slots, referenced in scrambled order -- by default an empty slot run, one visit, two visits at the same time, 40 visits (beyond any
    unroll or register cap) and an ordinary five.  30 % of the entries are missing at random, with NaN, inf and 1e300 (inf as a float32)
    written under every 0 mask byte; the last subject has no valid visit at vertex 0 and, with two vertices or more, exactly one at the
    last vertex.  With ten slots or more, one slot names row -1 and one row n_rows; the last offset lies beyond the slot count."""
    rng = np.random.default_rng(seed)
    E = int(sum(counts))
    R = E + 12
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    offsets[-1] += 7
    rows = rng.permutation(R)[:E].astype(np.int32)
    times = np.concatenate([np.sort(rng.uniform(0, 8, c)) for c in counts])
    for s, c in enumerate(counts):
        if c == 2:
            times[offsets[s] + 1] = times[offsets[s]]
    Y = rng.uniform(1, 4, (R, V)).astype(np.float32)
    mask = None
    if with_mask:
        mask = (rng.random((R, V)) > 0.3).astype(np.uint8)
        last = rows[offsets[-2]:E]
        mask[last, 0] = 0
        if V >= 2:
            mask[last, V - 1] = 0
            mask[last[len(last) // 2], V - 1] = 1
        with np.errstate(over="ignore"):
            garbage = np.array([np.nan, np.inf, 1e300]).astype(np.float32)
        Y[mask == 0] = garbage[np.arange(R * V).reshape(R, V) % 3][mask == 0]
    if E >= 10:
        rows[E // 4], rows[E // 2] = -1, R
    return Y, mask, offsets, rows, times, rng.uniform(0, 8, len(counts))
