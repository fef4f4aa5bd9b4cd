"""The cases of the vertex-wise design columns (include/oai_hip.h, "Vertex-wise design columns"): the shapes, the fixtures with their planted
corner cases, their restatement (tests/vertex_regression_ref.py) and the confound demonstration.  tests/test_vertex_regression_cpu.py
asserts on the restatement that the planted corners occur, so that the bit comparison of tests/test_vertex_regression_gpu.py on the same
fixtures cannot pass vacuously.  No tests and no fixtures here."""
import functools

import numpy as np

import group_regression_ref as rref
import group_stats_ref as gref
import vertex_regression_ref as vref
from cohort_cases import icosphere

# (p, s_n, s_i, k, intercept): k global columns are tested by F (0: the combination has a per-vertex regressor of interest and no F).
# The lone per-vertex x; p = 2 either way round; p = 4 with S = 1 and with S = 2 (both forms); p = 6 with S = 2 (both forms).
COMBOS = ((1, 0, 1, 0, False), (2, 1, 0, 1, False), (2, 0, 1, 0, True), (4, 1, 0, 2, True), (4, 1, 1, 0, True), (4, 2, 0, 1, True),
          (6, 2, 0, 2, True), (6, 1, 1, 0, True))
VERTS = (1, 63, 65, 257, 600)                     # both sides of a wave (64) and of a block's 256 vertices, several blocks
PLANTED = {"empty_w": 1, "dof0": 2, "dof1": 3, "constant_y": 4, "constant_w": 5, "complete": 6}


def knees(p):
    return (p + 1, 31, 65)


def rows_per_thread(p, S):                        # csrc/group_regression_vx.hip, rows_per_thread
    return {1: 8, 2: 8 if S == 1 else 4, 3: 2, 4: 2 if S == 1 else 4, 5: 2, 6: 2}[p]


def batch_rows(p, S):
    """One full row group and a ragged one."""
    r = rows_per_thread(p, S)
    return r + max(1, r // 4)


def row_counts(p, S):
    b = batch_rows(p, S)
    return (1, 2, b - 1, b + 1, 2 * b + 5)


def global_columns(N, p, s_n, s_i, k, intercept, rng):
    """[N, p - S]: the intercept (if any), continuous covariates, and last the columns of interest -- k 0 / 1 dummies of a factor with
    k + 1 levels, or (k = 1 without an intercept) one continuous regressor."""
    pg = p - s_n - s_i
    cols = [np.ones(N)] if intercept else []
    n_int = k if s_i == 0 else 0
    cols += [60 + 8 * rng.normal(0.0, 1.0, N) for _ in range(pg - len(cols) - n_int)]
    if n_int:
        level = np.arange(N) % (n_int + 1)
        cols += [(level == g).astype(np.float64) for g in range(1, n_int + 1)] if intercept else [rng.normal(0.0, 1.0, N)]
    assert len(cols) == pg
    return np.ascontiguousarray(np.stack(cols, axis=1)) if cols else np.zeros((N, 0))


@functools.lru_cache(maxsize=None)
def case(N, V, combo):
    """(Y float32 [N, V], mask, W float32 [S, N, V], wmask, global design [N, p - S], perm int32 [P, N]) with the corner cases planted where
    the shape has room (V >= 8)."""
    p, s_n, s_i, k, intercept = combo
    S = s_n + s_i
    rng = np.random.default_rng([N, V, p, s_n, s_i])
    D = global_columns(N, p, s_n, s_i, k, intercept, rng)
    W = (2.5 + 0.4 * rng.normal(size=(S, N, V))).astype(np.float32)
    Y = (2.0 + 0.5 * rng.normal(size=(N, V)) - 0.3 * (W[0] - 2.5) * rng.random(V)[None, :]).astype(np.float32)
    mask = rng.random((N, V)) >= 0.1
    wmask = rng.random((S, N, V)) >= 0.1
    P = max(row_counts(p, S))
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(P - 1)]).astype(np.int32)
    perm[1, 0], perm[1, N - 1] = -5, N + 3                                # out of range: clamped to knee 0 and knee N - 1
    mask[:, 0], wmask[:, :, 0] = True, True                               # an ordinary vertex
    if V >= 8:
        at = PLANTED
        wmask[0, :, at["empty_w"]] = False                                # w missing for every knee: n = 0
        for name, keep in (("dof0", p), ("dof1", p + 1)):
            mask[:, at[name]], wmask[:, :, at[name]] = np.arange(N) < keep, True
        Y[:, at["constant_y"]] = 0.0                                      # exactly constant: every residual is 0.0, s2 == 0
        W[0, :, at["constant_w"]] = 1.5                                   # constant over the complete cases: with an intercept, no pivot
        for name in ("constant_y", "constant_w"):
            mask[:, at[name]], wmask[:, :, at[name]] = True, True
        mask[:, at["complete"]] = True                                    # y valid everywhere, w missing at the first and the last knee: only w drops knees
        wmask[:, :, at["complete"]] = True
        wmask[S - 1, [0, N - 1], at["complete"]] = False
    W = np.where(wmask, W, np.float32(0.0))                               # as a cohort stores a missing entry
    for a in (Y, mask, W, wmask, D, perm):
        a.setflags(write=False)
    return Y, mask, W, wmask, D, perm


@functools.lru_cache(maxsize=None)
def reference(N, V, combo):
    """The restatement of a case: (prepared for t, t tile, slope0, prepared for F or None, F tile or None, coef0 or None)."""
    p, s_n, s_i, k, intercept = combo
    Y, mask, W, wmask, D, perm = case(N, V, combo)
    pg = D.shape[1]
    q_t = pg - (0 if s_i else 1)
    prep_t = vref.prepare(Y, mask, W, wmask, D[:, :q_t] if q_t else None, s_n, centre=intercept)
    t, slope = vref.regression_t(prep_t, D, perm, s_n, s_i, with_slope=True)
    out = [prep_t, t, slope, None, None, None]
    if k:
        prep_f = vref.prepare(Y, mask, W, wmask, D[:, :pg - k] if pg - k else None, s_n, centre=intercept)
        F, coef = vref.regression_f(prep_f, D, perm, s_n, k, with_coef=True)
        out[3:] = [prep_f, F, coef]
    for a in out:
        for b in (a.values() if isinstance(a, dict) else [a]):
            if b is not None:
                b.setflags(write=False)
    return tuple(out)


def planted_cases_occur(N, V, combo):
    """On the restatement: every corner case that was planted is really there."""
    p, s_n, s_i, k, intercept = combo
    Y, mask, W, wmask, D, perm = case(N, V, combo)
    prep, t, slope, prep_f, F, coef = reference(N, V, combo)
    at, m = PLANTED, prep["m"] != 0
    assert (mask & ~wmask.all(axis=0)).any() and (~mask & wmask.all(axis=0)).any()      # y valid where w is missing, and the reverse
    assert np.array_equal(prep["n"], (mask & wmask.all(axis=0)).sum(axis=0)) and np.array_equal(prep["n_dropped"], (mask & ~m).sum(axis=0))
    assert prep["n"][at["empty_w"]] == 0 and np.isnan(t[:, at["empty_w"]]).all() and (prep["WC"][:, :, at["empty_w"]] == 0.0).all()
    assert prep["n_dropped"][at["empty_w"]] == mask[:, at["empty_w"]].sum() > 0
    assert prep["n"][at["dof0"]] == p and np.isnan(t[:, at["dof0"]]).all() and np.isnan(slope[at["dof0"]])
    assert prep["n"][at["dof1"]] == p + 1 and prep["ok"][at["dof1"]] == 1 and not np.isnan(t[0, at["dof1"]]) and not np.isnan(slope[at["dof1"]])
    assert prep["Q"][at["constant_y"]] == 0.0 and prep["ok"][at["constant_y"]] == 1 and np.isnan(t[:, at["constant_y"]]).all()
    if intercept:
        assert prep["n"][at["constant_w"]] == N and np.isnan(t[:, at["constant_w"]]).all() and (prep["WC"][0, :, at["constant_w"]] == 0.0).all()
        assert prep["ok"][at["constant_w"]] == (0 if s_n else 1)          # a nuisance map fails in prepare, the lone x in the factor of M
    assert prep["n"][at["complete"]] == N - 2 and prep["n_dropped"][at["complete"]] == 2
    centred_fill = prep["WC"][-1, [0, N - 1], at["complete"]]
    assert (centred_fill == 0.0).all() if intercept or N == 2 else (centred_fill != 0.0).all()   # the completed value: exactly 0.0 when centred (and with n = 0)
    assert perm[1].min() < 0 and perm[1].max() >= N
    if N >= 31:
        assert not np.isnan(t[:, 0]).any() and not np.isnan(t[:, at["complete"]]).any()
        dealt_missing = ~wmask[-1][np.clip(perm, 0, N - 1)]                # [P, N, V]: knee j of the row is dealt a row whose w was missing
        assert (dealt_missing[1:] & m[None]).any(axis=(1, 2)).any()       # some row deals a valid knee a completed value
        assert not (dealt_missing[0] & m).any()                           # the identity never does
    if k:
        assert np.isnan(F[:, at["dof0"]]).all() and not np.isnan(F[0, at["dof1"]]) and (F[~np.isnan(F)] >= 0.0).all()
        assert np.isnan(coef[:, at["dof0"]]).all() and not np.isnan(coef[:, at["dof1"]]).any()


# ---- the confound that the per-vertex column removes ------------------------------------------------------------------------------------
CONFOUND_SEED, CONFOUND_N, CONFOUND_P, CONFOUND_BETA = 3, 24, 200, 0.05
CONFOUND_UNADJUSTED_CAP, CONFOUND_ADJUSTED = 43, 0         # vertices with p_fwer <= 0.05: inside the cap unadjusted; anywhere, adjusted


@functools.lru_cache(maxsize=None)
def confound():
    """Two groups of 12 knees on the sphere of test_group_f_gpu.py's end-to-end case.  Baseline thickness is 2.5 mm + 0.15 mm noise, and
    0.6 mm more in group 1 on the cap z > 0.8.  The rate is -beta (baseline - 2.5) + 0.01 mm / year noise: thick cartilage loses more, and
    NOTHING depends on the group.  10 % of the baseline and of the rate are missing, independently."""
    verts, _ = icosphere()
    cap = verts[:, 2] > 0.8
    rng = np.random.default_rng(CONFOUND_SEED)
    group = np.arange(CONFOUND_N) % 2
    rng.shuffle(group)
    base = 2.5 + 0.15 * rng.normal(size=(CONFOUND_N, len(verts)))
    base[np.ix_(group == 1, cap)] += 0.6
    base = base.astype(np.float32)
    rate = (-CONFOUND_BETA * (base.astype(np.float64) - 2.5) + 0.01 * rng.normal(size=base.shape)).astype(np.float32)
    mask, wmask = rng.random(base.shape) >= 0.1, rng.random(base.shape) >= 0.1
    return np.where(mask, rate, np.float32(0)), mask, np.where(wmask, base, np.float32(0)), wmask, group.astype(np.float64), cap


def confound_restated(adjusted: bool, index):
    """(t tile, p_fwer) of the group effect on the rate from the restatements, with the host's own design and p-values."""
    from oai_analysis_2_amd import stats
    rate, mask, base, wmask, group, cap = confound()
    Z, D, _ = rref.design_columns(group, None, True)
    if adjusted:
        t = vref.regression_t(vref.prepare(rate, mask, base[None], wmask[None], Z, 1), D, index, 1, 0)
    else:
        t = rref.regression_t(rref.prepare(rate, mask, Z), mask, D, index)
    max_abs, exceed = gref.reduce_tiles(t)
    return t, stats._p_values(t[0], max_abs, exceed, len(index))[1]
