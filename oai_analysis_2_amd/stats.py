"""Cohort statistics on atlas thickness maps: permutation tests, vertex by vertex, with a family-wise error over the whole surface.

The per-knee path ends in ``KneeThickness``: one float32 vector per cartilage on the atlas inner vertices, where the same vertex is the
same anatomical location in every knee.  This module takes N such vectors and says where two groups of knees differ
(``two_sample_test``: Student's pooled t under permutation of the group labels) or where a follow-up differs from baseline
(``paired_test``: one-sample t of the differences under sign flips).  The reference has no such step; the definitions are stated in
include/oai_hip.h ("Cohort statistics") and restated in tests/group_stats_ref.py.

Everything heavy runs on the device (csrc/group_stats.hip): P labellings x V vertices x N knees of fp64 adds in a fixed order, and one
connected-components pass over the atlas surface per labelling when a cluster threshold is given.  The p-values are formed on the host
from integer counts and the null distribution of max |t|, after ONE download at the end.  No significance level is built in: the result
holds p-values, and what counts as a finding is the study's decision.

    cohort = ThicknessCohort.from_stream(thickness_stream(...), atlas, "FC")
    res = two_sample_test(cohort, groups, n_permutations=10000, cluster_threshold=3.0)
    res.p_fwer, res.clusters, res.image(atlas, "t")

``regression_test`` asks how thickness varies with ONE continuous (or dummy) regressor, adjusted for nuisance covariates: the general
linear model per vertex, the t of the regressor's coefficient, Freedman-Lane permutation (include/oai_hip.h, "Cohort regression";
csrc/group_regression.hip; tests/group_regression_ref.py).

    res = regression_test(cohort, kl_grade, covariates=np.stack([age, sex], axis=1), n_permutations=10000, cluster_threshold=3.0)
    res.slope, res.partial_r, res.p_fwer

``f_test`` asks whether SEVERAL columns explain thickness jointly, and ``anova_test`` whether it differs across the levels of a factor (a
one-way analysis of variance, or of covariance with ``covariates``): the F of the last k design columns under the same permutation
scheme (include/oai_hip.h, "Cohort F test"; csrc/group_regression.hip; tests/group_f_ref.py).

    res = anova_test(cohort, kl_grade, covariates=age, n_permutations=10000, tfce=True)
    res.f, res.coefficients, res.group_mean, res.p_fwer

``tfce=True`` (or a ``TFCE``) on any of the tests adds threshold-free cluster enhancement (include/oai_hip.h, "Threshold-free cluster
enhancement"; csrc/graph_tfce.hip; tests/graph_tfce_ref.py): every labelling's t tile is integrated over all thresholds on the device and
``res.p_tfce`` is the family-wise p of the enhanced statistic -- sensitive to broad weak effects without a hand-picked threshold.

``cohort.smoothed(fwhm_mm=5.0)`` smooths every knee's map ALONG the atlas surface before any of the tests (include/oai_hip.h, "Surface
smoothing"; csrc/graph_smooth.hip; tests/graph_smooth_ref.py): iterated Gaussian-weighted neighbourhood averaging on the device that
neither reads nor invents a missing entry, with the sweep count calibrated on the mesh's own discrete kernel (``SurfaceSmoother``).

``LongitudinalCohort`` holds the visits of a longitudinal study -- several per knee, unevenly spaced, some missing -- and ``change`` fits a
straight line through each knee's own visits at every vertex on the device (include/oai_hip.h, "Longitudinal change";
csrc/visit_slopes.hip; tests/visit_slopes_ref.py).  The slopes are a ``ThicknessCohort`` again, one row per subject, for any of the tests
above and for ``one_sample_test``: is there loss at all, and where?

    visits = LongitudinalCohort.from_stream(thickness_stream(...), atlas, "FC", visits={index: (subject, years), ...})
    rate = visits.change("rate", min_visits=3)                          # mm / year per subject and vertex
    one_sample_test(rate, tfce=True).p_tfce, regression_test(rate, baseline_kl_grade).p_fwer

``NormativeModel`` answers the question about ONE knee: where is it abnormally thin for its age, sex and BMI, and is that more than chance
over the whole surface?  A linear model per vertex on a reference cohort, new knees scored by the prediction-interval t and the members
themselves by the externally studentised residual, per-knee family-wise p-values as ranks among the reference's own leave-one-out
statistics (include/oai_hip.h, "Normative deviation"; csrc/normative.hip; tests/normative_ref.py).

    model = NormativeModel.fit(healthy, covariates=np.stack([age, sex, bmi], axis=1), names=["age", "sex", "bmi"])
    res = model.deviation(knee_vector, covariates=[71.0, 1.0, 31.2], return_maps=True)
    res.p_max, res.area_below_mm2, res.clusters(0), res.image(atlas, "z")

``bootstrap_ci`` says how large an effect is, give or take what: the nonparametric bootstrap of the mean map, of an adjusted group
difference or of a slope, with percentile, basic or BCa intervals per vertex and a simultaneous sup-t band over the surface
(include/oai_hip.h, "Bootstrap intervals"; csrc/bootstrap.hip; tests/bootstrap_ref.py).

    ci = bootstrap_ci(rate, n_bootstrap=2000, method="bca", simultaneous=True)      # mm / year [lower, upper]
    ci.estimate, ci.lower, ci.upper, ci.lower_simultaneous, ci.image(atlas, "se")

``cohort.ranked()`` replaces every knee's value by its RANK among the knees that have a value at the vertex (or by the rank-based
inverse-normal score, or by Wilcoxon's signed rank) on the device, so that one mislabelled patch no longer inflates the variance of a
whole vertex (include/oai_hip.h, "Rank transform"; csrc/rank_transform.hip; tests/rank_transform_ref.py).  The result is a cohort again,
for any of the tests above; ``rank_sum_test``, ``signed_rank_test``, ``kruskal_test`` and ``spearman_test`` name the classical tests and
return their classical statistics beside the permutation result.

    res = rank_sum_test(cohort, groups, tfce=True)                                  # Mann-Whitney under permutation
    res.u1, res.auc, res.test.p_fwer, res.test.p_tfce
    signed_rank_test(rate).rank_biserial, two_sample_test(cohort.ranked("inormal"), groups).p_fwer

``cohort.pca()`` describes patterns over the whole surface and judges a knee against the cohort as a whole: an area-weighted,
missing-aware principal component analysis through the Gram matrix of the whitened knees, with Hotelling's T2 inside the model and the
residual Q outside it per knee (include/oai_hip.h, "Cohort PCA"; csrc/cohort_pca.hip; tests/cohort_pca_ref.py).

    pca = cohort.pca(10)                                                            # modes_mm, explained_variance_ratio, scores
    screen = pca.member_scores(); screen.q_fraction, screen.t2                      # a registration failure stands out in q
    regression_test(cohort, x=pca.scores[:, 0]), pca.transform(new_knee).q

``vertex_covariates=`` on ``regression_test``, ``f_test`` and ``anova_test`` puts MAPS into the design -- one number per knee and vertex,
baseline thickness at the same vertex above all, without which a rate of change regresses to the mean -- and ``x`` of ``regression_test``
may itself be a map (include/oai_hip.h, "Vertex-wise design columns"; csrc/group_regression_vx.hip; tests/vertex_regression_ref.py).

    regression_test(visits.change("rate"), x=kl_grade, covariates=np.stack([age, sex], axis=1), vertex_covariates=visits.first_visit()).p_fwer

Every test above takes the rows of a cohort as exchangeable.  ``marginal_test`` is the one-stage model for rows that come in CLUSTERS --
the visits of a subject, both knees of a subject: ordinary least squares over all rows, the cluster-robust (sandwich) t, and the wild
cluster bootstrap for its null distribution, so a covariate may vary within a subject (include/oai_hip.h, "Cluster-robust regression";
csrc/cluster_robust.hip; tests/cluster_robust_ref.py).

    g = visits.per_row(group)
    marginal_test(visits, x=visits.years * g, covariates=np.stack([visits.years, g], axis=1), tfce=True).p_tfce
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import mesh_processing as mp
from . import ops

WORKSPACE_BUDGET = 256 << 20          # bytes of t tile (and cluster labels) a default batch may take
_ROW_GROUP = 16                       # labellings per thread of the t kernel: a batch is a multiple of it


# ---- labellings ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Permutations:
    """``bits``: uint32 [P, ceil(N / 32)] -- knee i of row p is bit i % 32 of word i // 32; row 0 is the observed labelling.  ``exact``:
    the rows are ALL distinct labellings of the design, each once; otherwise rows 1.. are independent Monte Carlo draws, among which
    duplicates (and the observed labelling itself) may occur -- the p-values are the usual Monte Carlo estimates either way."""
    bits: np.ndarray
    n_knees: int
    exact: bool = False

    def __len__(self) -> int:
        return int(self.bits.shape[0])

    def rows(self) -> np.ndarray:
        """bool [P, N]."""
        return unpack_bits(self.bits, self.n_knees)


def pack_bits(rows) -> np.ndarray:
    """bool [P, N] -> uint32 [P, ceil(N / 32)]."""
    rows = np.atleast_2d(np.asarray(rows)).astype(bool)
    P, N = rows.shape
    padded = np.zeros((P, (N + 31) // 32 * 32), np.uint8)
    padded[:, :N] = rows
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(P, -1)


def unpack_bits(bits, n_knees: int) -> np.ndarray:
    """uint32 [P, ceil(N / 32)] -> bool [P, N]."""
    bits = np.ascontiguousarray(np.atleast_2d(bits), dtype="<u4")
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :int(n_knees)].astype(bool)


def _as_groups(groups) -> np.ndarray:
    g = np.asarray(groups)
    if g.ndim != 1 or g.dtype == object or not np.isin(g, (0, 1)).all():
        raise ValueError("groups must be one 0 / 1 (or bool) entry per knee: 1 = group 1, 0 = group 2")
    return g.astype(bool)


def _block_members(blocks, n_knees: int) -> List[np.ndarray]:
    """The knee indices of every block, ascending, in ascending block label; without ``blocks`` all knees are one block."""
    b = np.zeros(n_knees, np.int64) if blocks is None else np.asarray(blocks)
    if b.shape != (n_knees,):
        raise ValueError(f"blocks must hold one label per knee ({n_knees}), got shape {b.shape}")
    return [np.nonzero(b == lab)[0] for lab in np.unique(b)]


def label_permutations(groups, n_permutations: int, seed: int = 0, blocks=None) -> Permutations:
    """Labellings for ``two_sample_test``: row 0 is ``groups`` itself (1 / True = group 1), every other row a rearrangement of the labels
    that keeps both group sizes.  ``blocks``: an int label per knee (site, sex, ...); labels then move within a block only.  When the
    design has at most ``n_permutations`` distinct labellings they are all enumerated, each once (``exact``); otherwise rows 1.. are
    drawn from ``np.random.Generator(np.random.PCG64(seed))`` independently, so duplicates may occur."""
    g = _as_groups(groups)
    N, P = len(g), int(n_permutations)
    if P < 1:
        raise ValueError(f"n_permutations must be >= 1, got {n_permutations}")
    members = _block_members(blocks, N)
    total = math.prod(math.comb(len(idx), int(g[idx].sum())) for idx in members)
    if total <= P:
        rows = [g.copy()]
        per_block = [[np.asarray(c, np.int64) for c in itertools.combinations(range(len(idx)), int(g[idx].sum()))] for idx in members]
        for choice in itertools.product(*per_block):
            row = np.zeros(N, bool)
            for idx, c in zip(members, choice):
                row[idx[c]] = True
            if not np.array_equal(row, g):
                rows.append(row)
        return Permutations(pack_bits(np.stack(rows)), N, exact=True)
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.empty((P, N), bool)
    rows[0] = g
    for idx in members:
        rows[1:, idx] = rng.permuted(np.tile(g[idx], (P - 1, 1)), axis=1)
    return Permutations(pack_bits(rows), N)


def sign_flips(n_knees: int, n_permutations: int, seed: int = 0) -> Permutations:
    """Sign vectors for ``paired_test``: a set bit flips the knee's difference; row 0 flips nothing.  All 2^N vectors, each once, when
    there are at most ``n_permutations`` of them (``exact``); otherwise rows 1.. are independent draws from
    ``np.random.Generator(np.random.PCG64(seed))``, so duplicates may occur."""
    N, P = int(n_knees), int(n_permutations)
    if N < 1 or P < 1:
        raise ValueError(f"n_knees and n_permutations must be >= 1, got {n_knees}, {n_permutations}")
    if N < 62 and (1 << N) <= P:
        k = np.arange(1 << N, dtype=np.uint64)
        return Permutations(pack_bits((k[:, None] >> np.arange(N, dtype=np.uint64)) & np.uint64(1)), N, exact=True)
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.zeros((P, N), bool)
    rows[1:] = rng.integers(0, 2, size=(P - 1, N), dtype=np.uint8)
    return Permutations(pack_bits(rows), N)


# ---- the cohort matrix -----------------------------------------------------------------------------------------------------------------
class ThicknessCohort:
    """The knees of a study for one cartilage, as a float32 [N, V] matrix and its uint8 validity mask on the device, on the vertices of
    ``atlas.inner[kind]`` (a ``ThicknessAtlas``, or any object with its ``inner``, ``device`` and ``image``).  An entry is MISSING
    (mask 0) where the knee's value is NaN, in every entry of a cartilage listed in ``knee.errors``, and -- with ``use_coverage`` -- where
    ``knee.coverage[kind]`` is 0, so that denuded bone is missing rather than a thickness.  The matrix grows in chunks of ``chunk`` knees."""

    def __init__(self, atlas, kind: str, use_coverage: bool = False, chunk: int = 64):
        self.atlas, self.kind, self.use_coverage, self.chunk = atlas, kind, bool(use_coverage), max(int(chunk), 1)
        self.device = torch.device(atlas.device)
        self.n_verts = len(atlas.inner[kind].verts)
        self.ids: List[object] = []
        self._values = torch.zeros((0, self.n_verts), dtype=torch.float32, device=self.device)
        self._mask = torch.zeros((0, self.n_verts), dtype=torch.uint8, device=self.device)
        self._graph: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._areas: Optional[np.ndarray] = None
        self.smoothing: Optional["Smoothing"] = None       # set on the result of ``smoothed``
        self.change: Optional["Change"] = None             # set on the result of ``LongitudinalCohort.change``
        self.ranking: Optional["Ranking"] = None           # set on the result of ``ranked``

    def surface_graph(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The CSR vertex adjacency of the atlas inner mesh on the device (``mesh_processing.vertex_adjacency_device``), built at the
        first test that clusters and kept: it is the same for every test on this cohort."""
        if self._graph is None:
            faces = mp._dev(self.atlas.inner[self.kind].faces, np.int32, (3,), device=self.device)
            self._graph = mp.vertex_adjacency_device(self.n_verts, faces)
        return self._graph

    def vertex_areas(self) -> np.ndarray:
        """float64 [V]: ``mesh_processing.mesh_areas`` of the atlas inner mesh, in mm^2; computed once."""
        if self._areas is None:
            self._areas = mp.mesh_areas(self.atlas.inner[self.kind])[0]
        return self._areas

    def __len__(self) -> int:
        return len(self.ids)

    @property
    def values(self) -> torch.Tensor:
        return self._values[:len(self.ids)]

    @property
    def mask(self) -> torch.Tensor:
        return self._mask[:len(self.ids)]

    def _row(self) -> int:
        n = len(self.ids)
        if n == self._values.shape[0]:
            for name, dtype in (("_values", torch.float32), ("_mask", torch.uint8)):
                grown = torch.zeros((n + self.chunk, self.n_verts), dtype=dtype, device=self.device)
                grown[:n] = getattr(self, name)
                setattr(self, name, grown)
        return n

    def add_vector(self, vector, id=None, valid=None) -> None:
        """One knee as a bare vector [V] (array or device tensor; NaN = missing) with an optional validity vector."""
        vec = mp._dev(vector, np.float32, device=self.device).reshape(-1)
        if vec.numel() != self.n_verts:
            raise ValueError(f"the {self.kind} vector must have the atlas' {self.n_verts} vertices, got {vec.numel()}")
        ok = ~torch.isnan(vec)
        if valid is not None:
            ok &= mp._dev(valid, np.uint8, device=self.device).reshape(-1) != 0
        row = self._row()
        self._values[row] = torch.where(ok, vec, torch.zeros_like(vec))
        self._mask[row] = ok.to(torch.uint8)
        self.ids.append(len(self.ids) if id is None else id)

    def add(self, knee, id=None) -> None:
        """One ``KneeThickness`` (numpy or device vectors).  ``id``: what ``paired_test`` matches rows by; default, the row index."""
        if self.kind in knee.errors:
            self.add_vector(torch.full((self.n_verts,), float("nan")), id)
            return
        cover = knee.coverage.get(self.kind) if self.use_coverage else None
        if self.use_coverage and cover is None:
            raise ValueError(f"use_coverage needs knee.coverage[{self.kind!r}]: measure the knee with morphometry")
        self.add_vector(knee[self.kind], id, cover)

    @classmethod
    def from_stream(cls, stream: Iterable[Tuple[object, object]], atlas, kind: str, **kwargs) -> "ThicknessCohort":
        """Collect the (index, KneeThickness) pairs of ``thickness_stream`` / ``process_cohort_thickness``; the index is the knee's id."""
        cohort = cls(atlas, kind, **kwargs)
        for index, knee in stream:
            cohort.add(knee, index)
        return cohort

    def summary(self) -> dict:
        """Per vertex: ``n`` (knees with a value), ``mean``, ``std`` (n - 1 in the denominator; NaN below two knees), as arrays."""
        if len(self) < 2:
            raise ValueError("a summary needs at least two knees")
        prep = ops.group_prepare(self.values, self.mask)
        return {"n": prep.n.cpu().numpy(), "mean": prep.mean.cpu().numpy(), "std": prep.std.cpu().numpy()}

    def smoothed(self, fwhm_mm: Optional[float] = None, *, sweeps: Optional[int] = None, sigma_step: Optional[float] = None,
                 missing: str = "keep", batch: Optional[int] = None) -> "ThicknessCohort":
        """A NEW cohort on the same atlas, cartilage and ids whose maps are these smoothed along the atlas surface (``SurfaceSmoother``,
        whose arguments these are: exactly one of ``fwhm_mm`` and ``sweeps``); this cohort is untouched.  The float32 values are widened
        to float64 (exact), all sweeps run in float64 on the device, and the result is rounded to float32 once at the end.  Knees go
        through in batches of ``batch`` rows -- default ``smoothing_batch``, so that the workspace stays within ``WORKSPACE_BUDGET``.  ``missing="keep"``: an
        entry that is missing stays missing; "fill": it takes the average of what surrounds it, ring by ring.  The settings are kept on
        the result as ``.smoothing`` (a ``Smoothing``); the three tests take the result as they take any cohort."""
        _check_smoothing_arguments(fwhm_mm, sweeps, sigma_step, missing)
        N, V = len(self), self.n_verts
        if N < 1:
            raise ValueError("the cohort holds no knee to smooth")
        smoother = SurfaceSmoother(self.atlas, self.kind, fwhm_mm, sweeps=sweeps, sigma_step=sigma_step, missing=missing, graph=self.surface_graph())
        out = ThicknessCohort(self.atlas, self.kind, self.use_coverage, self.chunk)
        out.ids, out._graph, out._areas, out.smoothing, out.change = list(self.ids), self._graph, self._areas, smoother.settings, self.change
        out._values = torch.zeros((N, V), dtype=torch.float32, device=self.device)
        out._mask = torch.zeros((N, V), dtype=torch.uint8, device=self.device)
        rows = smoothing_batch(V, N) if batch is None else int(batch)
        if rows < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        for r0 in range(0, N, rows):
            r1 = min(r0 + rows, N)
            wide = self.values[r0:r1].to(torch.float64)
            smoother.smooth_tile(wide, self.mask[r0:r1], out=wide, out_mask=out._mask[r0:r1])
            out._values[r0:r1] = wide.to(torch.float32)
        return out

    def _derived_like(self, values: torch.Tensor, mask: torch.Tensor) -> "ThicknessCohort":
        """A new cohort on this one's atlas, cartilage, ids and graph with ``.smoothing`` and ``.change`` carried over, as ``smoothed``
        builds its result, holding the float32 ``values`` and uint8 ``mask`` [N, V]."""
        out = ThicknessCohort(self.atlas, self.kind, self.use_coverage, self.chunk)
        out.ids, out._graph, out._areas, out.smoothing, out.change = list(self.ids), self._graph, self._areas, self.smoothing, self.change
        out._values, out._mask = values, mask
        return out

    def _ranked(self, method: str, c) -> Tuple["ThicknessCohort", "ops.ColumnRanks"]:
        """``ranked`` and the ranks it was made from, which the four rank tests take their classical statistics from."""
        if self.ranking is not None:
            raise ValueError(f"this cohort is already ranked ({self.ranking.method!r}): ranks of ranks are the same ranks, and normal scores of "
                             "normal scores are not what anyone means")
        if method not in _RANK_METHODS:
            raise ValueError(f"method must be one of {sorted(_RANK_METHODS)}, got {method!r}")
        if len(self) < 1:
            raise ValueError("the cohort holds no knee to rank")
        signed, kind = _RANK_METHODS[method]
        constant = rank_constant(c)
        ranks = ops.column_ranks(self.values, self.mask, signed=signed)
        score, mask = ops.rank_scores(ranks.twice_rank, ranks.n_valid, kind, constant)
        out = self._derived_like(score.to(torch.float32), mask)
        out.ranking = Ranking(method, constant if kind == "normal" else None, ranks.n_valid, ranks.tie_term)
        return out, ranks

    def ranked(self, method: str = "rank", c="blom") -> "ThicknessCohort":
        """A NEW cohort on the same atlas, cartilage and ids whose values are scores of the RANKS of these, taken per vertex among the
        knees that have a value there (include/oai_hip.h, "Rank transform"; csrc/rank_transform.hip; tests/rank_transform_ref.py); this
        cohort is untouched, and ``.smoothing`` and ``.change`` are carried over.  ``method``:
          "rank"            the midrank (ties share the average of their ranks), exact in float32;
          "centred"         the midrank minus (n + 1) / 2, n the knees with a value at the vertex; exact;
          "inormal"         the rank-based inverse-normal transform Phi^-1((r - c) / (n - 2 c + 1)), computed in float64 and rounded
                            to float32 once;
          "signed"          Wilcoxon's signed ranks: the midrank of |value| with the value's sign; a value of exactly zero is dropped
                            before ranking and BECOMES MISSING in the result;
          "signed_inormal"  the normal score of the signed rank's size, with the value's sign.
        ``c``: "blom" (3/8, the default, as recalled from PALM's -inormal and pinned to no implementation), "tukey" (1/3), "rankit"
        (1/2, Bliss), "waerden" (0), or a number in [0, 1/2]; read by the two inormal methods alone.  The result's mask is the
        transform's; it carries ``.ranking`` (a ``Ranking``), and every test takes it as it takes a smoothed cohort.  Ranking a cohort
        that is already ranked is refused.  Ranks are taken over the whole cohort: the tests' ``blocks`` restrict the permutations and
        never the ranking."""
        return self._ranked(method, c)[0]

    def difference(self, other: "ThicknessCohort") -> "ThicknessCohort":
        """A NEW cohort holding this cohort minus ``other`` within a knee: rows are matched by id exactly as ``paired_test`` matches them
        (every id of either cohort in the other, once), the row order and ids are this cohort's, the difference a - b is taken on the
        device in float32 and is missing where either side is.  ``.smoothing`` and ``.change`` are carried over where both sides agree
        on them."""
        if self.kind != other.kind or self.n_verts != other.n_verts or self.device != other.device:
            raise ValueError("the two cohorts must hold the same cartilage of the same atlas on the same GPU")
        where_b = {id_: k for k, id_ in enumerate(other.ids)}
        if len(where_b) != len(other) or len(set(self.ids)) != len(self) or set(self.ids) != set(where_b):
            raise ValueError("difference needs the same ids in both cohorts, each once")
        if self.ranking is not None or other.ranking is not None:
            raise ValueError("a difference of ranks is not a rank: take the difference first, then rank it")
        order = torch.tensor([where_b[id_] for id_ in self.ids], dtype=torch.int64, device=self.device)
        mask = self.mask * other.mask.index_select(0, order)
        out = self._derived_like((self.values - other.values.index_select(0, order)) * mask, mask)      # missing entries hold 0 on either side
        out.smoothing = self.smoothing if self.smoothing == other.smoothing else None
        out.change = self.change if self.change == other.change else None
        return out

    def pca(self, n_components: int = 10, weights="area", min_valid: int = 2) -> "ThicknessPCA":
        """``ThicknessPCA.fit(self, ...)``: the modes of variation of this cohort's maps and its knees' outlier scores (T2 inside the
        model, Q outside it).  On a derived cohort the settings travel with the model: ``cohort.ranked("inormal").pca()`` is the
        correlation-type analysis."""
        return ThicknessPCA.fit(self, n_components, weights, min_valid)


# ---- surface smoothing -----------------------------------------------------------------------------------------------------------------
_FWHM_PER_SIGMA = math.sqrt(8.0 * math.log(2.0))
_SMOOTH_BYTES = 8 + 1 + 18            # per (knee, vertex) of a batch: the float64 tile, its mask and oai_graph_smooth_workspace_bytes


@dataclass(frozen=True)
class Smoothing:
    """What a smoothed cohort was smoothed with: the nominal ``fwhm_mm`` (None when the sweeps were given), the ``achieved_fwhm_mm`` that
    the mesh's own discrete kernel amounts to after ``sweeps`` sweeps, the ``sigma_step`` (mm) of the edge weights, and ``missing``."""
    fwhm_mm: Optional[float]
    achieved_fwhm_mm: float
    sweeps: int
    sigma_step: float
    missing: str


RANK_CONSTANTS = {"blom": 0.375, "tukey": 1.0 / 3.0, "rankit": 0.5, "waerden": 0.0}
_RANK_METHODS = {"rank": (False, "rank"), "centred": (False, "centred"), "inormal": (False, "normal"), "signed": (True, "rank"),
                 "signed_inormal": (True, "normal")}          # method -> (signed ranks, the kind of ops.rank_scores)


def rank_constant(c) -> float:
    """The constant c of the normal score Phi^-1((r - c) / (n - 2 c + 1)): one of ``RANK_CONSTANTS`` by name, or a number in [0, 1/2]."""
    if isinstance(c, str):
        if c not in RANK_CONSTANTS:
            raise ValueError(f"c must be one of {sorted(RANK_CONSTANTS)} or a number in [0, 1/2], got {c!r}")
        return RANK_CONSTANTS[c]
    c = float(c)
    if not 0.0 <= c <= 0.5:
        raise ValueError(f"c must lie in [0, 1/2], got {c!r}")
    return c


@dataclass(frozen=True)
class Ranking:
    """What a ranked cohort was ranked with: the ``method`` of ``ThicknessCohort.ranked``, the constant ``c`` of its normal scores (None
    for the methods without), and per vertex, as DEVICE tensors [V], ``n_valid`` int32 -- the knees that were ranked there -- and
    ``tie_term`` int64, the sum over the tie groups of t^3 - t."""
    method: str
    c: Optional[float]
    n_valid: torch.Tensor
    tie_term: torch.Tensor


def _csr_slots(offsets, neighbours, n_verts: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(owner, neighbour, slot) of every CSR slot that the kernel reads: offsets clamped into [0, E], neighbours outside [0, V) left out."""
    off, nbr = np.asarray(offsets, np.int64).reshape(-1), np.asarray(neighbours, np.int64).reshape(-1)
    V, E = int(n_verts), len(nbr)
    if len(off) != V + 1:
        raise ValueError(f"offsets must hold {V + 1} entries, got {len(off)}")
    lo, hi = np.clip(off[:-1], 0, E), np.clip(off[1:], 0, E)
    count = np.maximum(hi - lo, 0)
    owner = np.repeat(np.arange(V, dtype=np.int64), count)
    slot = np.repeat(lo - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    ok = (nbr[slot] >= 0) & (nbr[slot] < V)
    return owner[ok], nbr[slot][ok], slot[ok]


def surface_edge_d2(verts, offsets, neighbours) -> np.ndarray:
    """float64 [E]: the squared length of every directed edge of the CSR adjacency, dx*dx + dy*dy + dz*dz added left to right on the
    coordinates promoted to float64; 0.0 in a slot that the kernel does not read."""
    v = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    owner, nbr, slot = _csr_slots(offsets, neighbours, len(v))
    d = v[nbr] - v[owner]
    d2 = np.zeros(len(np.asarray(neighbours).reshape(-1)), np.float64)
    d2[slot] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return d2


def mean_edge_length(verts, offsets, neighbours) -> float:
    """The mean length of the directed edges of the mesh: the default ``sigma_step``."""
    _, _, slot = _csr_slots(offsets, neighbours, len(np.asarray(verts).reshape(-1, 3)))
    if len(slot) == 0:
        raise ValueError("the mesh has no edge")
    return float(np.sqrt(surface_edge_d2(verts, offsets, neighbours)[slot]).mean())


def surface_edge_weights(verts, offsets, neighbours, sigma_step: float) -> np.ndarray:
    """float64 [E], aligned with ``neighbours``: w = exp(-d2 / (2 * sigma_step**2)) per directed edge, d2 as ``surface_edge_d2``; the self
    weight that goes with it is 1, the same Gaussian at distance 0.  0.0 in a slot that the kernel does not read."""
    sigma_step = float(sigma_step)
    if not (sigma_step > 0.0 and math.isfinite(sigma_step)):
        raise ValueError(f"sigma_step must be finite and > 0, got {sigma_step!r}")
    _, _, slot = _csr_slots(offsets, neighbours, len(np.asarray(verts).reshape(-1, 3)))
    d2 = surface_edge_d2(verts, offsets, neighbours)
    w = np.zeros_like(d2)
    w[slot] = np.exp(-d2[slot] / (2 * sigma_step ** 2))
    return w


def surface_step_variance(offsets, neighbours, weights, d2) -> np.ndarray:
    """float64 [V]: s_i = sum_j w_ij d2_ij / (1 + sum_j w_ij), the second moment of ONE sweep's kernel around vertex i (self weight 1).
    0.0 for a vertex without a neighbour."""
    V = len(np.asarray(offsets).reshape(-1)) - 1
    owner, _, slot = _csr_slots(offsets, neighbours, V)
    w, d2 = np.asarray(weights, np.float64).reshape(-1), np.asarray(d2, np.float64).reshape(-1)
    if len(w) != len(d2) or len(w) != len(np.asarray(neighbours).reshape(-1)):
        raise ValueError("weights and d2 must be aligned with neighbours")
    return np.bincount(owner, w[slot] * d2[slot], minlength=V) / (1.0 + np.bincount(owner, w[slot], minlength=V))


def sweeps_for_fwhm(fwhm_mm: float, step_variance, has_neighbour=None) -> int:
    """The number K of sweeps whose kernel has the second moment of a Gaussian of ``fwhm_mm``: sigma = fwhm / sqrt(8 ln 2), K = 2 sigma^2
    / s_mean rounded half to even, at least 1.  ``step_variance``: ``surface_step_variance`` (or one number, s_mean itself); s_mean is
    its plain mean over the vertices that have a neighbour (``has_neighbour`` bool [V]; default: those with s_i > 0).  On a regular
    lattice the second moment of the impulse response after K sweeps is exactly K s, because the variances of the steps add: the only
    error left is the rounding of K.  On an irregular mesh s varies from vertex to vertex and the calibration is approximate."""
    fwhm_mm = float(fwhm_mm)
    if not (fwhm_mm > 0.0 and math.isfinite(fwhm_mm)):
        raise ValueError(f"fwhm_mm must be finite and > 0, got {fwhm_mm!r}")
    s_mean = _mean_step_variance(step_variance, has_neighbour)
    sigma = fwhm_mm / _FWHM_PER_SIGMA
    ratio = 2.0 * sigma * sigma / s_mean
    if not math.isfinite(ratio) or round(ratio) > ops.MAX_SMOOTH_SWEEPS:
        raise ValueError(f"a FWHM of {fwhm_mm} mm needs about {ratio:.0f} sweeps of this step, more than {ops.MAX_SMOOTH_SWEEPS}: "
                         "give a larger sigma_step")
    return max(int(round(ratio)), 1)


def _mean_step_variance(step_variance, has_neighbour=None) -> float:
    s = np.atleast_1d(np.asarray(step_variance, np.float64))
    keep = s > 0.0 if has_neighbour is None else np.asarray(has_neighbour, bool)
    if not keep.any() or not float(s[keep].mean()) > 0.0:
        raise ValueError("the step variance is 0 everywhere: the graph has no edge of positive length and weight")
    return float(s[keep].mean())


def _check_smoothing_arguments(fwhm_mm, sweeps, sigma_step, missing) -> None:
    """Refuses what the smoother would, before anything is looked at or launched."""
    if (fwhm_mm is None) == (sweeps is None):
        raise ValueError("give exactly one of fwhm_mm and sweeps")
    if missing not in ("keep", "fill"):
        raise ValueError(f'missing must be "keep" or "fill", got {missing!r}')
    if fwhm_mm is not None and not (float(fwhm_mm) > 0.0 and math.isfinite(float(fwhm_mm))):
        raise ValueError(f"fwhm_mm must be finite and > 0, got {fwhm_mm!r}")
    if sweeps is not None and not 1 <= int(sweeps) <= ops.MAX_SMOOTH_SWEEPS:
        raise ValueError(f"sweeps must be 1 .. {ops.MAX_SMOOTH_SWEEPS}, got {sweeps!r}")
    if sigma_step is not None and not (float(sigma_step) > 0.0 and math.isfinite(float(sigma_step))):
        raise ValueError(f"sigma_step must be finite and > 0, got {sigma_step!r}")


def smoothing_batch(n_verts: int, n_rows: int, budget: int = WORKSPACE_BUDGET) -> int:
    """Knees per batch of ``ThicknessCohort.smoothed``: what fits ``budget`` bytes -- per (knee, vertex) 8 of float64 tile, 1 of mask and
    the 18 of the kernel's transposed ping and pong -- at least one."""
    return int(min(max(budget // (int(n_verts) * _SMOOTH_BYTES), 1), max(int(n_rows), 1)))


class SurfaceSmoother:
    """Smoothing of scalar fields ALONG the inner surface of ``atlas.inner[kind]`` (include/oai_hip.h, "Surface smoothing";
    csrc/graph_smooth.hip): K sweeps of Gaussian-weighted neighbourhood averaging over the mesh edges, the weight of an edge being
    exp(-d^2 / (2 sigma_step^2)) of its length d and that of the vertex itself 1.  Exactly one of ``fwhm_mm`` (then K =
    ``sweeps_for_fwhm``, calibrated on this mesh's own step variance) and ``sweeps`` is given.  ``sigma_step`` (mm): default, the mean
    edge length.  ``missing``: "keep" -- a missing entry stays missing and gives nothing to its neighbours; "fill" -- it takes the
    average of its valid neighbours, ring by ring.  ``graph``: the (offsets, neighbours) device tensors of
    ``ThicknessCohort.surface_graph()``, to share them; default: built here.  The graph, the weights and K are formed once and the
    weights uploaded once.  ``fwhm_mm`` is the nominal figure; ``achieved_fwhm_mm`` = sqrt(8 ln 2 * K s_mean / 2) is what K whole sweeps
    amount to.  Distances are edge lengths, not geodesics, and on an irregular mesh the calibration is approximate: ``impulse`` shows the
    kernel that is actually applied."""

    def __init__(self, atlas, kind: str, fwhm_mm: Optional[float] = None, *, sweeps: Optional[int] = None, sigma_step: Optional[float] = None,
                 missing: str = "keep", graph: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        _check_smoothing_arguments(fwhm_mm, sweeps, sigma_step, missing)
        mesh = atlas.inner[kind]
        self.atlas, self.kind, self.missing = atlas, kind, missing
        self.device = torch.device(atlas.device)
        self.n_verts = len(mesh.verts)
        if graph is None:
            graph = mp.vertex_adjacency_device(self.n_verts, mp._dev(mesh.faces, np.int32, (3,), device=self.device))
        self.graph = graph
        off, nbr = graph[0].cpu().numpy(), graph[1].cpu().numpy()
        self.sigma_step = mean_edge_length(mesh.verts, off, nbr) if sigma_step is None else float(sigma_step)
        weights = surface_edge_weights(mesh.verts, off, nbr, self.sigma_step)
        s = surface_step_variance(off, nbr, weights, surface_edge_d2(mesh.verts, off, nbr))
        owner, _, slot = _csr_slots(off, nbr, self.n_verts)
        has_neighbour = np.bincount(owner, minlength=self.n_verts) > 0
        self.step_variance = _mean_step_variance(s, has_neighbour)
        self.fwhm_mm = None if fwhm_mm is None else float(fwhm_mm)
        self.sweeps = int(sweeps) if fwhm_mm is None else sweeps_for_fwhm(fwhm_mm, s, has_neighbour)
        self.achieved_fwhm_mm = math.sqrt(8.0 * math.log(2.0) * self.sweeps * self.step_variance / 2.0)
        self.weights = torch.from_numpy(weights).to(self.device)
        self._vertex_sum = 1.0 + np.bincount(owner, weights[slot], minlength=self.n_verts)      # d_i of ``impulse``

    @property
    def settings(self) -> Smoothing:
        return Smoothing(self.fwhm_mm, self.achieved_fwhm_mm, self.sweeps, self.sigma_step, self.missing)

    def smooth_tile(self, values: torch.Tensor, mask: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                    out_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``ops.graph_smooth`` of a float64 device tile [R, V] and its uint8 mask with this smoother's graph, weights and sweeps."""
        return ops.graph_smooth(values, self.graph[0], self.graph[1], self.weights, mask=mask, sweeps=self.sweeps, fill=self.missing == "fill",
                                out=out, out_mask=out_mask)

    def __call__(self, field, valid=None):
        """One knee [V] or a matrix [N, V], numpy or a device tensor, NaN = missing (``valid``: also missing where it is 0) -> the same
        kind, shape and floating dtype, smoothed in float64 and NaN where the result is missing."""
        is_tensor = isinstance(field, torch.Tensor)
        if is_tensor:
            dtype = field.dtype if field.dtype.is_floating_point else torch.float64
        else:
            dtype = np.asarray(field).dtype if np.asarray(field).dtype.kind == "f" else np.dtype(np.float64)
        x = (field.to(self.device) if is_tensor else torch.from_numpy(np.ascontiguousarray(field, dtype=np.float64)).to(self.device)).to(torch.float64)
        if x.dim() not in (1, 2) or x.shape[-1] != self.n_verts or x.numel() == 0:
            raise ValueError(f"the field must be [{self.n_verts}] or [N >= 1, {self.n_verts}], got {tuple(x.shape)}")
        tile = x.reshape(-1, self.n_verts).contiguous()
        ok = ~torch.isnan(tile)
        if valid is not None:
            ok &= mp._dev(valid, np.uint8, device=self.device).reshape(tile.shape) != 0
        N = int(tile.shape[0])
        out, out_mask = torch.empty_like(tile), torch.empty(tile.shape, dtype=torch.uint8, device=self.device)
        mask = ok.to(torch.uint8)
        rows = smoothing_batch(self.n_verts, N)
        for r0 in range(0, N, rows):
            r1 = min(r0 + rows, N)
            self.smooth_tile(tile[r0:r1], mask[r0:r1], out=out[r0:r1], out_mask=out_mask[r0:r1])
        out = torch.where(out_mask != 0, out, torch.full_like(out, float("nan"))).reshape(x.shape)
        return out.to(dtype) if is_tensor else out.cpu().numpy().astype(dtype)

    def impulse(self, vertex: int) -> np.ndarray:
        """float64 [V]: the kernel that is actually applied at ``vertex`` with nothing missing -- entry j is the weight with which the
        smoothed value at ``vertex`` averages the input at j, so the entries are >= 0 and sum to 1.  It is formed as the response to an
        impulse: with d_i = 1 + sum_j w_ij and symmetric edge weights, the response at i to a value 1 / d_vertex at ``vertex``, times d_i.
        Where every vertex has the same d (a regular mesh) that IS the response to a unit value at ``vertex``; elsewhere the response
        differs from it by the factor d_vertex / d_i."""
        vertex = int(vertex)
        if not 0 <= vertex < self.n_verts:
            raise ValueError(f"vertex must be in [0, {self.n_verts}), got {vertex}")
        unit = torch.zeros((1, self.n_verts), dtype=torch.float64, device=self.device)
        unit[0, vertex] = 1.0 / float(self._vertex_sum[vertex])
        return self.smooth_tile(unit, None)[0][0].cpu().numpy() * self._vertex_sum


# ---- longitudinal change ---------------------------------------------------------------------------------------------------------------
VisitSlopes = ops.VisitSlopes
CHANGE_MEASURES = {"rate": ("rate",), "avg": ("avg",), "pc1": ("rate", "fit_ref"), "spc": ("rate", "avg")}     # what each reads of the fit


@dataclass
class VisitTable:
    """The visits of a study grouped by subject, as ``ops.visit_slopes`` takes them: ``subjects`` in order of first appearance; subject s
    owns the slots ``offsets[s] .. offsets[s+1] - 1`` (int32 [S+1]) of ``rows`` (int32 [E]: the position of the visit in the input) and
    ``times`` (float64 [E]: its years), in ascending time with ties in input order; ``reference_time`` float64 [S]."""
    subjects: List[object]
    offsets: np.ndarray
    rows: np.ndarray
    times: np.ndarray
    reference_time: np.ndarray


def visit_table(subjects, years, reference="first") -> VisitTable:
    """Group visits by subject: ``subjects[i]`` (any hashable) and ``years[i]`` (a float, years since whatever origin the study uses)
    describe visit i.  ``reference``: the time at which a subject's fitted value is read off (``fit_ref``, the denominator of "pc1") --
    "first": the subject's earliest visit over ALL its visits, not only those valid at a vertex; a float: the same time for every
    subject; a mapping from subject to time.  Refuses a time that is not finite and a (subject, time) pair given twice."""
    subjects = list(subjects)
    times = np.asarray(years, np.float64).reshape(-1)
    if len(times) != len(subjects):
        raise ValueError(f"subjects and years must hold one entry per visit, got {len(subjects)} and {len(times)}")
    index: dict = {}
    owner = np.array([index.setdefault(s, len(index)) for s in subjects], np.int64)
    names = list(index)
    for i in np.nonzero(~np.isfinite(times))[0][:1]:
        raise ValueError(f"the time of visit {int(i)} of subject {subjects[i]!r} is not finite: {float(times[i])!r}")
    order = np.lexsort((np.arange(len(times)), times, owner))              # by subject, then time, then input order
    same = (owner[order][1:] == owner[order][:-1]) & (times[order][1:] == times[order][:-1])
    for k in np.nonzero(same)[0][:1]:
        raise ValueError(f"subject {subjects[order[k]]!r} has two visits at {float(times[order[k]])!r} years (visits {int(order[k])} and {int(order[k + 1])})")
    S = len(names)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=S))]).astype(np.int32)
    sorted_times = times[order]
    if isinstance(reference, str):
        if reference != "first":
            raise ValueError(f'reference must be "first", a time or a mapping from subject to time, got {reference!r}')
        tref = sorted_times[offsets[:-1]] if S else np.zeros(0)
    elif hasattr(reference, "keys"):
        missing = [s for s in names if s not in reference]
        if missing:
            raise ValueError(f"reference has no time for subject {missing[0]!r}")
        tref = np.array([float(reference[s]) for s in names], np.float64)
    else:
        tref = np.full(S, float(reference), np.float64)
    if not np.isfinite(tref).all():
        raise ValueError(f"the reference time of subject {names[int(np.nonzero(~np.isfinite(tref))[0][0])]!r} is not finite")
    return VisitTable(names, offsets, order.astype(np.int32), sorted_times, np.ascontiguousarray(tref, np.float64))


@dataclass(frozen=True)
class Change:
    """What a cohort of ``LongitudinalCohort.change`` holds: the ``measure`` ("rate" mm / year, "avg" mm, "pc1" or "spc" % / year), the
    least number of valid visits and the least span in years a fit needed, and the ``reference`` time ("first", a float, or "per subject"
    for a mapping)."""
    measure: str
    min_visits: int
    min_span_years: float
    reference: object


class LongitudinalCohort:
    """The visits of a longitudinal study for one cartilage: every row is one knee at one visit, with the subject it belongs to and the
    time of the visit in years.  The rows live in a ``ThicknessCohort`` (``.rows``), so MISSING means exactly what it means there: NaN, an
    errored cartilage, or -- with ``use_coverage`` -- denuded bone.  Subjects may have different numbers of visits at different times.

    ``change`` is stage one of the two-stage (summary-measures) analysis: a straight line through each subject's own visits at every
    vertex (include/oai_hip.h, "Longitudinal change"; csrc/visit_slopes.hip), and the slopes come back as a ``ThicknessCohort`` with one
    row per subject that ``one_sample_test`` (is there loss at all?), ``two_sample_test``, ``regression_test``, ``f_test`` and
    ``anova_test`` (in whom is it faster?) take like any other.  A vertex that is missing in some of a subject's visits is fitted through
    the others.  Smoothing may come before the fit (``smoothed``: every visit's map) or after it (``change(...).smoothed(...)``: the
    rate maps); smoothing and fitting are both linear, so the two agree where nothing is missing, and differ where entries are missing:
    before, a missing entry leaves its neighbours' averages in that visit alone; after, it has already changed n and the slope at its own
    vertex."""

    def __init__(self, atlas, kind: str, use_coverage: bool = False, chunk: int = 64):
        self.rows = ThicknessCohort(atlas, kind, use_coverage, chunk)
        self._subject: List[object] = []
        self._years: List[float] = []
        self._label: List[object] = []
        self._seen: set = set()

    atlas = property(lambda self: self.rows.atlas)
    kind = property(lambda self: self.rows.kind)
    device = property(lambda self: self.rows.device)
    n_verts = property(lambda self: self.rows.n_verts)

    def __len__(self) -> int:
        return len(self._subject)

    def _note(self, subject, years) -> float:
        years = float(years)
        if not math.isfinite(years):
            raise ValueError(f"the time of a visit of subject {subject!r} is not finite: {years!r}")
        if (subject, years) in self._seen:
            raise ValueError(f"subject {subject!r} already has a visit at {years!r} years")
        return years

    def _noted(self, subject, years: float, visit) -> None:
        self._seen.add((subject, years))
        self._subject.append(subject)
        self._years.append(years)
        self._label.append(visit)

    def add_vector(self, vector, subject, years, valid=None, visit=None) -> None:
        """One knee at one visit as a bare vector [V] (NaN = missing) with an optional validity vector; ``visit``: a label ("V03")."""
        years = self._note(subject, years)
        self.rows.add_vector(vector, (subject, years), valid)
        self._noted(subject, years, visit)

    def add(self, knee, subject, years, visit=None) -> None:
        """One ``KneeThickness`` of ``subject`` at ``years``."""
        years = self._note(subject, years)
        self.rows.add(knee, (subject, years))
        self._noted(subject, years, visit)

    @classmethod
    def from_stream(cls, stream: Iterable[Tuple[object, object]], atlas, kind: str, visits, **kwargs) -> "LongitudinalCohort":
        """Collect the (index, KneeThickness) pairs of ``thickness_stream`` / ``process_cohort_thickness``; ``visits[index]`` (or
        ``visits(index)``) is the knee's (subject, years) or (subject, years, label)."""
        cohort = cls(atlas, kind, **kwargs)
        for index, knee in stream:
            cohort.add(knee, *(visits(index) if callable(visits) else visits[index]))
        return cohort

    @classmethod
    def from_cohorts(cls, cohorts, **kwargs) -> "LongitudinalCohort":
        """From one ``ThicknessCohort`` per visit, ``{years: cohort, ...}``: a cohort's ids are the subjects, its rows their knees at that
        time.  The cohorts must hold the same cartilage of the same atlas on the same GPU; their rows are copied."""
        cohorts = dict(cohorts)
        if not cohorts:
            raise ValueError("from_cohorts needs at least one cohort")
        first = next(iter(cohorts.values()))
        out = cls(first.atlas, first.kind, kwargs.pop("use_coverage", first.use_coverage), kwargs.pop("chunk", first.chunk), **kwargs)
        for years, c in cohorts.items():
            if c.kind != out.kind or c.n_verts != out.n_verts or c.device != out.device:
                raise ValueError("the cohorts must hold the same cartilage of the same atlas on the same GPU")
            for i, subject in enumerate(c.ids):
                out.add_vector(c.values[i], subject, years, valid=c.mask[i])
        return out

    @property
    def subjects(self) -> List[object]:
        """In order of first appearance: the ids of what ``change`` returns."""
        return list(dict.fromkeys(self._subject))

    @property
    def years(self) -> np.ndarray:
        """float64 [rows]: the time of every row in years, in the order the rows were added -- a per-row column for ``marginal_test``."""
        return np.asarray(self._years, np.float64)

    def per_row(self, values) -> np.ndarray:
        """A per-SUBJECT quantity (group, sex, baseline age) broadcast to the rows, in the order the rows were added: ``values`` is an
        array with one entry (or one row of entries) per subject in the order of ``subjects``, or a mapping from subject to value."""
        if hasattr(values, "keys"):
            missing = [s for s in self.subjects if s not in values]
            if missing:
                raise ValueError(f"per_row has no value for subject {missing[0]!r}")
            return np.asarray([values[s] for s in self._subject])
        names = self.subjects
        values = np.asarray(values)
        if values.ndim < 1 or values.shape[0] != len(names):
            raise ValueError(f"per_row needs one entry per subject ({len(names)}, in the order of subjects) or a mapping, got shape {values.shape}")
        where = {s: k for k, s in enumerate(names)}
        return values[np.asarray([where[s] for s in self._subject], np.int64)]

    def visits_of(self, subject) -> List[Tuple[float, object]]:
        """The (years, label) of the subject's visits in ascending time."""
        return sorted(((y, lab) for s, y, lab in zip(self._subject, self._years, self._label) if s == subject), key=lambda p: p[0])

    def at_visit(self, visit) -> ThicknessCohort:
        """The rows of one visit as a ``ThicknessCohort`` whose ids are the subjects -- what ``paired_test`` matches rows by: the rows
        labelled ``visit``, or, where no row carries that label, those at ``visit`` years.  A copy."""
        picked = [i for i, lab in enumerate(self._label) if lab is not None and lab == visit]
        if not picked and isinstance(visit, (int, float)) and not isinstance(visit, bool):
            picked = [i for i, y in enumerate(self._years) if y == float(visit)]
        if not picked:
            raise ValueError(f"no row is labelled or timed {visit!r}")
        ids = [self._subject[i] for i in picked]
        if len(set(ids)) != len(ids):
            raise ValueError(f"a subject has more than one row at visit {visit!r}")
        return self._derived(ids, *(t.index_select(0, torch.tensor(picked, dtype=torch.int64, device=self.device))
                                    for t in (self.rows.values, self.rows.mask)))

    def first_visit(self) -> ThicknessCohort:
        """Every subject's EARLIEST row as a ``ThicknessCohort`` whose ids are ``subjects`` (so the rows match those of ``change``), missing
        where that row is -- baseline thickness at the same vertex, the adjustment a rate of change needs against regression to the mean:
        ``regression_test(visits.change("rate"), x=kl_grade, covariates=np.stack([age, sex], axis=1), vertex_covariates=visits.first_visit())``.  A copy."""
        if not len(self):
            raise ValueError("the cohort holds no visit")
        table = visit_table(self._subject, self._years)
        picked = torch.from_numpy(table.rows[table.offsets[:-1]].astype(np.int64)).to(self.device)
        return self._derived(table.subjects, self.rows.values.index_select(0, picked), self.rows.mask.index_select(0, picked))

    def _derived(self, ids, values: torch.Tensor, mask: torch.Tensor) -> ThicknessCohort:
        out = ThicknessCohort(self.atlas, self.kind, self.rows.use_coverage, self.rows.chunk)
        out.ids, out._graph, out._areas, out.smoothing = list(ids), self.rows._graph, self.rows._areas, self.rows.smoothing
        out._values, out._mask = values.contiguous(), mask.contiguous()
        return out

    def smoothed(self, *args, **kwargs) -> "LongitudinalCohort":
        """A NEW longitudinal cohort whose every visit is smoothed along the atlas surface (``ThicknessCohort.smoothed``, whose arguments
        these are): smoothing BEFORE the fit."""
        out = LongitudinalCohort.__new__(LongitudinalCohort)
        out.rows = self.rows.smoothed(*args, **kwargs)
        out._subject, out._years, out._label, out._seen = list(self._subject), list(self._years), list(self._label), set(self._seen)
        return out

    def trajectories(self, min_visits: int = 2, min_span_years: float = 0.0, reference="first", want: Sequence[str] = ops.SLOPE_OUTPUTS) -> VisitSlopes:
        """``ops.visit_slopes`` of the rows grouped by ``visit_table``: the fits of every subject (in the order of ``subjects``) at every
        vertex, on the device.  A fit exists where at least ``min_visits`` visits are valid at the vertex and span at least
        ``min_span_years``.  ``reference``: as in ``visit_table``."""
        if not len(self):
            raise ValueError("the cohort holds no visit")
        table = visit_table(self._subject, self._years, reference)
        dev = self.device
        return ops.visit_slopes(self.rows.values, *(torch.from_numpy(a).to(dev) for a in (table.offsets, table.rows, table.times, table.reference_time)),
                                mask=self.rows.mask, min_visits=min_visits, min_span=min_span_years, want=want)

    def change(self, measure: str = "rate", min_visits: int = 2, min_span_years: float = 0.0, reference="first") -> ThicknessCohort:
        """A NEW ``ThicknessCohort`` with one row per subject (ids = ``subjects``): "rate", the fitted slope in mm / year; "avg", the mean
        over the valid visits in mm; "pc1", the rate in per cent of the fitted value at the reference time, 100 * rate / fit_ref; "spc", in
        per cent of the mean, 100 * rate / avg (both % / year; the quotient is taken in float64 on the device, rate / denominator first and
        times 100 after, and the entry is missing where the denominator is not > 0).  An entry is missing where the subject has no fit at
        the vertex (``trajectories``).  The float64 plane is rounded to float32 once.  The settings are kept on the result as ``.change``
        (a ``Change``)."""
        if measure not in CHANGE_MEASURES:
            raise ValueError(f"measure must be one of {tuple(CHANGE_MEASURES)}, got {measure!r}")
        reads = CHANGE_MEASURES[measure]
        fits = self.trajectories(min_visits, min_span_years, reference, want=tuple(dict.fromkeys(reads + ("mask",))))
        ok, plane = fits.mask != 0, getattr(fits, reads[0])
        if len(reads) == 2:
            den = getattr(fits, reads[1])
            ok = ok & (den > 0)
            plane = (plane / torch.where(ok, den, torch.ones_like(den))) * 100.0
        out = self._derived(self.subjects, torch.where(ok, plane, torch.zeros_like(plane)).to(torch.float32), ok.to(torch.uint8))
        kept = reference if isinstance(reference, str) else ("per subject" if hasattr(reference, "keys") else float(reference))
        out.change = Change(measure, int(min_visits), float(min_span_years), kept)
        return out


# ---- the tests -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TFCE:
    """The settings of threshold-free cluster enhancement (include/oai_hip.h): the step ``dh`` of the threshold in units of t, the exponents
    ``E`` (0.5 or 1) of the extent and ``H`` (1 or 2) of the height, what ``extent`` is -- "area": mm^2 of the atlas inner surface, kept
    as integers in units of 2^-20 mm^2; "vertices": a count -- and ``max_steps``, the number of levels after which the integral is cut
    (``tfce_clipped`` reports it).  The defaults are the surface defaults of PALM as recalled (E = 1, H = 2, area)."""
    dh: float = 0.1
    E: float = 1.0
    H: float = 2.0
    extent: str = "area"
    max_steps: int = 1000


_TFCE_AREA_UNIT = 2.0 ** -20          # mm^2 per unit of integer vertex weight: a power of two, so weight * unit is exact
_TFCE_BYTES = 8 + 16                  # per (labelling, vertex): the TFCE tile and oai_graph_tfce_workspace_bytes


def _tfce_settings(tfce) -> Optional[TFCE]:
    """None / False -> None, True -> the defaults, a ``TFCE`` -> itself; refuses what the kernel would, before anything is launched."""
    if tfce is None or tfce is False:
        return None
    settings = TFCE() if tfce is True else tfce
    if not isinstance(settings, TFCE):
        raise ValueError(f"tfce must be None, True or a TFCE, got {tfce!r}")
    if settings.E not in (0.5, 1.0) or settings.H not in (1.0, 2.0):
        raise ValueError(f"TFCE: E must be 0.5 or 1 and H must be 1 or 2, got E = {settings.E!r}, H = {settings.H!r}")
    if not (isinstance(settings.dh, (int, float)) and settings.dh > 0.0 and math.isfinite(settings.dh)):
        raise ValueError(f"TFCE: dh must be finite and > 0, got {settings.dh!r}")
    if settings.extent not in ("area", "vertices"):
        raise ValueError(f'TFCE: extent must be "area" or "vertices", got {settings.extent!r}')
    if not 1 <= int(settings.max_steps) <= 65536:
        raise ValueError(f"TFCE: max_steps must be 1 .. 65536, got {settings.max_steps!r}")
    return settings


def tfce_weights(areas: np.ndarray) -> np.ndarray:
    """int64 [V]: vertex areas in mm^2 as integers in units of 2^-20 mm^2 (round half to even), what ``extent="area"`` sums."""
    weights = np.rint(np.asarray(areas, np.float64) * 2.0 ** 20).astype(np.int64)
    if not (weights >= 0).all() or not sum(weights.tolist()) < 2 ** 53:          # Python ints: no wrap
        raise ValueError("TFCE: the vertex areas must be >= 0 and sum to less than 2^53 units of 2^-20 mm^2")
    return weights


@dataclass
class Cluster:
    label: int               # the cluster's smallest vertex index: its value in ``cluster_label``
    sign: int                # +1: t > threshold, -1: t < -threshold
    extent: int              # vertices
    area: float              # mm^2 of the atlas inner surface (vertex areas summed in ascending vertex index)
    p_cluster: float         # share of labellings whose largest cluster has at least this extent


@dataclass(kw_only=True)
class _SurfaceResult:
    """What the results of the three tests share: the cluster and TFCE fields (keyword-only, after the test's own fields) and ``image``,
    which takes the names in ``IMAGES``.  A result class declares its own fields -- ``kind``, the cartilage, among them -- and ``IMAGES``."""
    cluster_threshold: Optional[float] = None
    cluster_label: Optional[np.ndarray] = None
    clusters: List[Cluster] = field(default_factory=list)
    max_extent: Optional[np.ndarray] = None
    tfce: Optional[np.ndarray] = None
    p_tfce: Optional[np.ndarray] = None
    p_tfce_uncorrected: Optional[np.ndarray] = None
    max_tfce: Optional[np.ndarray] = None
    tfce_clipped: int = 0
    tfce_settings: Optional["TFCE"] = None

    IMAGES = ()

    def image(self, atlas, what: str = "t"):
        """``atlas.image`` of one of the result's ``IMAGES`` (float32 [H, W], NaN off the surface) -- of a ``PermutationResult``: "t", "p_fwer",
        "p_uncorrected", "mean_difference", "cluster_label", "tfce" or "p_tfce"; of a ``RegressionResult``: "t", "slope", "partial_r",
        "p_fwer", "p_uncorrected", "n", "cluster_label", "tfce" or "p_tfce"; of an ``FResult``: "f", "partial_eta2", "p_fwer",
        "p_uncorrected", "n", "cluster_label", "tfce" or "p_tfce"."""
        if what not in self.IMAGES:
            raise ValueError(f"no image of {what!r}")
        vec = getattr(self, what)
        if vec is None:
            raise ValueError("the test ran without tfce" if "tfce" in what else "the test ran without a cluster threshold")
        return atlas.image(np.asarray(vec, np.float32), self.kind)


@dataclass
class PermutationResult(_SurfaceResult):
    """``t`` float64 [V] (NaN where no t exists: fewer than two knees on a side, or no variance); ``n1``, ``n2`` the knees with a value
    per vertex and side (paired: both the number of pairs); ``mean_difference`` group 1 - group 2 (paired: mean of a - b);
    ``p_uncorrected`` = share of labellings with |t| at least the observed at that vertex; ``p_fwer`` = share of labellings whose max |t|
    over the surface is at least the observed |t| at that vertex (both NaN where t is); ``max_abs`` the null distribution of max |t|,
    one entry per labelling, entry 0 observed.  With a cluster threshold: ``cluster_label`` int32 [V] (-1 outside every cluster),
    ``clusters`` in ascending label, ``max_extent`` the null distribution of the largest cluster's extent.  With ``tfce``: ``tfce`` float64
    [V], the enhanced statistic with the sign of t (NaN where t is); ``p_tfce`` = share of labellings whose max |TFCE| over the surface is
    at least the observed |TFCE| at that vertex, ``p_tfce_uncorrected`` the vertex-wise share; ``max_tfce`` the null distribution of
    max |TFCE|; ``tfce_clipped`` the number of labellings with a vertex whose |t| reached past ``max_steps`` levels (0 unless t is huge or
    infinite: raise ``max_steps`` or ``dh`` otherwise); ``tfce_settings`` the ``TFCE`` that was used."""
    kind: str
    t: np.ndarray
    n1: np.ndarray
    n2: np.ndarray
    mean_difference: np.ndarray
    p_uncorrected: np.ndarray
    p_fwer: np.ndarray
    max_abs: np.ndarray
    n_permutations: int
    exact: bool

    IMAGES = ("t", "p_fwer", "p_uncorrected", "mean_difference", "cluster_label", "tfce", "p_tfce")


def _batch_rows(n_verts: int, n_permutations: int, clusters: bool, tfce: bool, budget: int, row_bytes: int = 0) -> int:
    """Rows per batch: what fits ``budget`` bytes of workspace -- per row 8 bytes per vertex of t tile, 8 more of labels and sizes with
    clusters, 24 more of TFCE tile and union-find with ``tfce``, and ``row_bytes`` of the test's own -- rounded down to sixteen rows (a
    multiple of every rows-per-thread of the t kernels), at least sixteen."""
    rows = budget // (int(n_verts) * ((16 if clusters else 8) + (_TFCE_BYTES if tfce else 0)) + row_bytes)
    return int(min(max(rows // _ROW_GROUP * _ROW_GROUP, _ROW_GROUP), max(int(n_permutations), 1)))


def default_batch(n_verts: int, n_permutations: int, clusters: bool, budget: int = WORKSPACE_BUDGET, tfce: bool = False) -> int:
    """Labellings per batch of ``two_sample_test`` and ``paired_test``: ``_batch_rows`` with nothing of the test's own per row."""
    return _batch_rows(n_verts, n_permutations, clusters, tfce, budget)


def _download(tensors: Sequence[torch.Tensor]) -> List[np.ndarray]:
    """Every tensor in one device-to-host copy."""
    flat = torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in tensors]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        out.append(flat[off:off + nbytes].view(getattr(np, str(t.dtype).split(".")[1])).reshape(tuple(t.shape)).copy())
        off += nbytes
    return out


class _Batches:
    """The batches of one test: the device side of what the three tests share -- the graph, the TFCE weights (uploaded once), the running
    results -- then the loop over ``rows`` rows at a time, ONE download, and the result fields that do not depend on the test.
    ``row_bytes``: what a row of a batch takes beyond its tiles, for the default of ``batch`` (``_batch_rows``)."""

    def __init__(self, cohort_like, P: int, V: int, dev, cluster_threshold: Optional[float], tfce: Optional[TFCE], batch: Optional[int],
                 row_bytes: int = 0):
        if cluster_threshold is not None and not float(cluster_threshold) > 0.0:
            raise ValueError(f"cluster_threshold must be > 0, got {cluster_threshold!r}")
        rows = _batch_rows(V, P, cluster_threshold is not None, tfce is not None, WORKSPACE_BUDGET, row_bytes) if batch is None else int(batch)
        if rows < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        self.cohort, self.P, self.V, self.dev, self.rows = cohort_like, P, V, dev, min(rows, P)
        self.threshold, self.tfce = cluster_threshold, tfce
        self.graph = cohort_like.surface_graph() if cluster_threshold is not None or tfce is not None else None

        def empty(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)

        self.out = {"t": empty(V, torch.float64), "max_abs": empty(P, torch.float64), "exceed": empty(V, torch.int64)}
        if cluster_threshold is not None:
            self.out["max_extent"] = empty(P, torch.int32)
        if tfce is not None:
            self.weights, self.unit = None, 1.0
            if tfce.extent == "area":
                self.weights, self.unit = torch.from_numpy(tfce_weights(cohort_like.vertex_areas())).to(dev), _TFCE_AREA_UNIT
            self.tfce_tile = empty((self.rows, V), torch.float64)
            self.out.update(tfce=empty(V, torch.float64), max_tfce=empty(P, torch.float64), tfce_exceed=empty(V, torch.int64),
                            tfce_clipped=empty(P, torch.int32))

    def run(self, tile_of, extras) -> Tuple[dict, dict]:
        """Queues every batch without a synchronisation -- ``tile_of(p0, p1)``: the float64 [p1 - p0, V] t tile of rows [p0, p1), then the
        reduce, the clusters and the TFCE of that tile -- and downloads once.  Returns the host arrays by name (the running results and
        ``extras``, a dict of named device tensors to bring along) and the keyword arguments of the result that every test shares."""
        out, P, graph, s = self.out, self.P, self.graph, self.tfce
        with torch.cuda.device(self.dev):
            for p0 in range(0, P, self.rows):
                p1 = min(p0 + self.rows, P)
                tile = tile_of(p0, p1)
                ops.permutation_reduce(tile, p0, out["t"], out["max_abs"], out["exceed"])
                if self.threshold is not None:
                    got = ops.graph_clusters(tile, graph[0], graph[1], float(self.threshold), max_extent=out["max_extent"][p0:p1],
                                             return_labels=p0 == 0)
                    if p0 == 0:
                        _, out["label"], out["size"] = got
                if s is not None:
                    enhanced, _ = ops.graph_tfce(tile, graph[0], graph[1], dh=s.dh, E=s.E, H=s.H, weights=self.weights, unit=self.unit,
                                                 max_steps=int(s.max_steps), out=self.tfce_tile[:p1 - p0], clipped=out["tfce_clipped"][p0:p1])
                    ops.permutation_reduce(enhanced, p0, out["tfce"], out["max_tfce"], out["tfce_exceed"])
            names = list(out) + list(extras)
            assert len(set(names)) == len(names), f"an extra tensor takes the name of a running result: {sorted(extras)}"
            host = dict(zip(names, _download([*out.values(), *extras.values()])))
        return host, self._fields(host)

    def _fields(self, host: dict) -> dict:
        t, P = host["t"], self.P
        p_unc, p_fwer = _p_values(t, host["max_abs"], host["exceed"], P)
        res = dict(t=t, p_uncorrected=p_unc, p_fwer=p_fwer, max_abs=host["max_abs"], n_permutations=P)
        if self.threshold is not None:
            label, size, area = host["label"], host["size"], self.cohort.vertex_areas()
            extents = np.sort(host["max_extent"])
            clusters = []
            for lab in np.unique(label[label >= 0]):
                members = np.nonzero(label == lab)[0]                          # ascending vertex index
                extent = int(size[lab])
                clusters.append(Cluster(int(lab), 1 if t[lab] > 0 else -1, extent, float(np.cumsum(area[members])[-1]),
                                        float(P - np.searchsorted(extents, extent, side="left")) / float(P)))
            res.update(cluster_threshold=float(self.threshold), cluster_label=label, max_extent=host["max_extent"], clusters=clusters)
        if self.tfce is not None:
            p_tfce_unc, p_tfce = _p_values(host["tfce"], host["max_tfce"], host["tfce_exceed"], P)
            res.update(tfce=host["tfce"], max_tfce=host["max_tfce"], tfce_clipped=int(np.count_nonzero(host["tfce_clipped"])), tfce_settings=self.tfce,
                       p_tfce_uncorrected=p_tfce_unc, p_tfce=p_tfce)
        return res


def _p_values(t: np.ndarray, max_abs: np.ndarray, exceed: np.ndarray, P: int) -> Tuple[np.ndarray, np.ndarray]:
    """(p_uncorrected, p_fwer) from the integer counts and the null distribution of max |t|; NaN where t is.  A row whose t is NaN at a
    vertex counts as not exceeding there: the denominator is P all the same."""
    valid = ~np.isnan(t)
    p_unc = np.where(valid, exceed / float(P), np.nan)
    null = np.sort(max_abs)
    p_fwer = np.where(valid, (P - np.searchsorted(null, np.abs(np.where(valid, t, 0.0)), side="left")) / float(P), np.nan)
    return p_unc, p_fwer


def _bit_tiles(cohort_like, values: torch.Tensor, mask: Optional[torch.Tensor], perms: Permutations, mode: int, cluster_threshold, tfce, batch):
    """What ``two_sample_test`` and ``paired_test`` share: the ``_Batches`` of the labellings ``perms``, the prepared block of ``values``
    and the function that makes a batch's t tile from them in one reused workspace."""
    N, V = int(values.shape[0]), int(values.shape[1])
    if perms.n_knees != N:
        raise ValueError(f"the labellings are for {perms.n_knees} knees, the cohort has {N}")
    dev = values.device
    batches = _Batches(cohort_like, len(perms), V, dev, cluster_threshold, tfce, batch)
    bits = torch.from_numpy(np.ascontiguousarray(perms.bits).view(np.int32)).to(dev)
    prepared = ops.group_prepare(values, mask, centre=mode == ops.STATS_TWO_SAMPLE)
    ws = _lib.workspace("oai_permutation_t", dev, batches.rows, V)
    return batches, prepared, lambda p0, p1: ops.permutation_t(prepared, bits, p0, p1, mode, workspace=ws)


def _permutations(perms, make, n_knees: int) -> Permutations:
    if perms is None:
        return make()
    if isinstance(perms, Permutations):
        return perms
    bits = np.asarray(perms)
    if bits.dtype == bool:
        bits = pack_bits(bits)
    return Permutations(np.ascontiguousarray(bits, dtype=np.uint32), n_knees)


def two_sample_test(cohort: ThicknessCohort, groups, n_permutations: int = 10000, cluster_threshold: Optional[float] = None, seed: int = 0,
                    blocks=None, permutations=None, batch: Optional[int] = None, tfce=None) -> PermutationResult:
    """Where do the knees of group 1 (``groups[i]`` = 1) differ from those of group 2 (= 0)?  Student's pooled t per vertex; its null
    distribution comes from ``label_permutations(groups, n_permutations, seed, blocks)``, or from ``permutations`` -- a ``Permutations``,
    packed uint32 rows or bool [P, N] with the observed labelling as row 0 -- for designs that does not cover.  ``cluster_threshold``
    (a |t| value): also clusters of supra-threshold vertices on the atlas surface and their extent-based p-values.  ``batch``: labellings
    per launch; default ``default_batch``.  ``tfce``: True or a ``TFCE`` adds threshold-free cluster enhancement of every labelling's t
    and the ``tfce`` fields of the result; it may be given together with ``cluster_threshold``.  A vertex where a group has fewer than two
    knees with a value has no t (NaN)."""
    tfce = _tfce_settings(tfce)
    g = _as_groups(groups)
    if len(g) != len(cohort):
        raise ValueError(f"groups must hold one entry per knee of the cohort ({len(cohort)}), got {len(g)}")
    if g.sum() < 2 or (~g).sum() < 2:
        raise ValueError("each group needs at least two knees")
    perms = _permutations(permutations, lambda: label_permutations(g, n_permutations, seed, blocks), len(g))
    if not np.array_equal(perms.rows()[0], g):
        raise ValueError("row 0 of the permutations must be the observed labelling")
    values, mask = cohort.values, cohort.mask
    sides = {}
    for side, member in (("1", g), ("2", ~g)):                             # the descriptive side: n and mean of either group, per vertex
        idx = torch.from_numpy(np.nonzero(member)[0]).to(values.device)
        prep = ops.group_prepare(values.index_select(0, idx), mask.index_select(0, idx))
        sides.update({"n" + side: prep.n, "mean" + side: prep.mean})
    batches, _, tile_of = _bit_tiles(cohort, values, mask, perms, ops.STATS_TWO_SAMPLE, cluster_threshold, tfce, batch)
    host, shared = batches.run(tile_of, sides)
    return PermutationResult(kind=cohort.kind, n1=host["n1"], n2=host["n2"], mean_difference=host["mean1"] - host["mean2"], exact=perms.exact,
                             **shared)


def paired_test(cohort_a: ThicknessCohort, cohort_b: ThicknessCohort, n_permutations: int = 10000, cluster_threshold: Optional[float] = None,
                seed: int = 0, permutations=None, batch: Optional[int] = None, tfce=None) -> PermutationResult:
    """Where does ``cohort_a`` differ from ``cohort_b`` within a knee (follow-up against baseline)?  Rows are matched by id (every id of
    either cohort must be in the other, once); the difference a - b is taken on the device and is missing where either side is; the
    statistic is the one-sample t of the differences and its null distribution comes from ``sign_flips``.  ``tfce``: as in
    ``two_sample_test``."""
    tfce = _tfce_settings(tfce)
    if cohort_a.kind != cohort_b.kind or cohort_a.n_verts != cohort_b.n_verts or cohort_a.device != cohort_b.device:
        raise ValueError("the two cohorts must hold the same cartilage of the same atlas on the same GPU")
    where_b = {id_: k for k, id_ in enumerate(cohort_b.ids)}
    if len(where_b) != len(cohort_b) or len(set(cohort_a.ids)) != len(cohort_a) or set(cohort_a.ids) != set(where_b):
        raise ValueError("paired_test needs the same ids in both cohorts, each once")
    N = len(cohort_a)
    if N < 2:
        raise ValueError("paired_test needs at least two pairs")
    order = torch.tensor([where_b[id_] for id_ in cohort_a.ids], dtype=torch.int64, device=cohort_a.device)
    mask = cohort_a.mask * cohort_b.mask.index_select(0, order)
    diff = (cohort_a.values - cohort_b.values.index_select(0, order)) * mask        # missing entries hold 0 on either side
    return _one_sample(cohort_a, diff, mask, n_permutations, cluster_threshold, seed, permutations, batch, tfce)


def _one_sample(cohort_like, values: torch.Tensor, mask: torch.Tensor, n_permutations: int, cluster_threshold, seed: int, permutations, batch,
                tfce: Optional[TFCE]) -> PermutationResult:
    """What ``paired_test`` and ``one_sample_test`` share: the one-sample t of the rows of ``values`` under sign flips."""
    N = int(values.shape[0])
    perms = _permutations(permutations, lambda: sign_flips(N, n_permutations, seed), N)
    if perms.rows()[0].any():
        raise ValueError("row 0 of the permutations must flip nothing")
    batches, prepared, tile_of = _bit_tiles(cohort_like, values, mask, perms, ops.STATS_ONE_SAMPLE, cluster_threshold, tfce, batch)
    host, shared = batches.run(tile_of, {"n": prepared.n, "mean": prepared.mean})
    return PermutationResult(kind=cohort_like.kind, n1=host["n"], n2=host["n"].copy(), mean_difference=host["mean"], exact=perms.exact, **shared)


def one_sample_test(cohort: ThicknessCohort, n_permutations: int = 10000, cluster_threshold: Optional[float] = None, seed: int = 0,
                    permutations=None, batch: Optional[int] = None, tfce=None) -> PermutationResult:
    """Where do the cohort's own values differ from zero -- of a rate cohort (``LongitudinalCohort.change``): is there loss at all, and
    where?  The one-sample t of the values per vertex; its null distribution comes from ``sign_flips`` (under the null a subject's change is
    as likely to be a gain as a loss), or from ``permutations`` with a first row that flips nothing.  It is ``paired_test`` of the cohort
    against zeros, without the zeros: ``n1`` = ``n2`` = the subjects with a value at the vertex, ``mean_difference`` their mean.
    ``cluster_threshold``, ``batch`` and ``tfce``: as in ``two_sample_test``."""
    tfce = _tfce_settings(tfce)
    if len(cohort) < 2:
        raise ValueError("one_sample_test needs at least two knees")
    return _one_sample(cohort, cohort.values, cohort.mask, n_permutations, cluster_threshold, seed, permutations, batch, tfce)


# ---- regression ------------------------------------------------------------------------------------------------------------------------
@dataclass
class IndexPermutations:
    """``index``: int32 [P, N] -- knee j of row p takes the design row ``index[p, j]``; row 0 is the identity.  ``exact``: the rows are ALL
    permutations of the design (within blocks), each once, in lexicographic order; otherwise rows 1.. are independent Monte Carlo draws."""
    index: np.ndarray
    exact: bool = False

    def __len__(self) -> int:
        return int(self.index.shape[0])


def index_permutations(n_knees: int, n_permutations: int, seed: int = 0, blocks=None) -> IndexPermutations:
    """Index rows for ``regression_test``: row 0 the identity, every other row a permutation of 0 .. N - 1.  ``blocks``: an int label per
    knee (site, sex, ...); knees then move within a block only.  When there are at most ``n_permutations`` such permutations (the product
    of n_b! over the blocks) they are all enumerated, each once, in lexicographic order (``exact``); otherwise rows 1.. are drawn from
    ``np.random.Generator(np.random.PCG64(seed)).permuted`` independently, so duplicates (and the identity) may occur."""
    N, P = int(n_knees), int(n_permutations)
    if N < 1 or P < 1:
        raise ValueError(f"n_knees and n_permutations must be >= 1, got {n_knees}, {n_permutations}")
    members = _block_members(blocks, N)
    total = 1
    for idx in members:
        total *= math.factorial(len(idx)) if total <= P else 1             # stop multiplying once it is beyond P
    if total <= P:
        rows = []
        for choice in itertools.product(*[itertools.permutations(idx.tolist()) for idx in members]):
            row = np.empty(N, np.int32)
            for idx, c in zip(members, choice):
                row[idx] = c
            rows.append(row)
        return IndexPermutations(np.stack(rows), exact=True)               # the first product is the identity
    rng = np.random.Generator(np.random.PCG64(seed))
    index = np.tile(np.arange(N, dtype=np.int32), (P, 1))
    for idx in members:
        index[1:, idx] = rng.permuted(np.tile(idx.astype(np.int32), (P - 1, 1)), axis=1)
    return IndexPermutations(index)


@dataclass
class RegressionResult(_SurfaceResult):
    """``t`` float64 [V]: the t of the regressor's coefficient (NaN where no t exists: too few knees with a value, a design that loses its
    rank among them, no residual variance); ``n`` the knees with a value and ``dof`` = n - p per vertex; ``slope`` in mm per unit of ``x``;
    ``partial_r`` = t / sqrt(t^2 + dof), the partial correlation of thickness and x given the covariates; the p-values, ``max_abs`` and the
    cluster and TFCE fields as in ``PermutationResult``."""
    kind: str
    t: np.ndarray
    n: np.ndarray
    dof: np.ndarray
    slope: np.ndarray
    partial_r: np.ndarray
    p_uncorrected: np.ndarray
    p_fwer: np.ndarray
    max_abs: np.ndarray
    n_permutations: int
    exact: bool

    IMAGES = ("t", "slope", "partial_r", "p_fwer", "p_uncorrected", "n", "cluster_label", "tfce", "p_tfce")
    # With per-vertex design columns (``vertex_covariates``, or ``x`` as a map): int32 [V], the knees with a value at the vertex that a
    # missing covariate dropped -- ``n`` and ``dof`` then count the complete cases.  None otherwise; set on the instance, not a field.
    n_dropped = None


def _table_bytes(n_knees: int, n_columns: int) -> int:
    """Per index row, the permuted design table of ``oai_regression_t``: 8 (p + p (p + 1) / 2) bytes per knee."""
    p = int(n_columns)
    return int(n_knees) * 8 * (p + p * (p + 1) // 2)


def regression_batch(n_verts: int, n_knees: int, n_columns: int, n_permutations: int, clusters: bool, budget: int = WORKSPACE_BUDGET,
                     tfce: bool = False) -> int:
    """Index rows per batch of ``regression_test``: ``_batch_rows`` with the row's ``_table_bytes`` of permuted design table."""
    return _batch_rows(n_verts, n_permutations, clusters, tfce, budget, _table_bytes(n_knees, n_columns))


def _n_columns(columns) -> int:
    """How many columns a host side of a design passes: None has none, [N] is one, [N, k] are k."""
    return 0 if columns is None else (1 if np.ndim(columns) == 1 else int(np.shape(columns)[-1]))


def _design_matrix(X, covariates, intercept: bool, n_knees: int, names: Optional[Sequence[str]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The one place that centres, scales and rank-checks the host columns of a design: (nuisance [N, q], design [N, q + k] with the k
    columns of ``X`` last, the k scales those columns were divided by); refuses what has no answer and names the column at fault
    (``names``: what the columns of ``X`` are called; default "X column j").  ``X`` None: no tested column among them (k = 0: the
    regressor of interest is a map) and the design is the nuisance."""
    tested = X is not None
    X = np.asarray(X, np.float64) if tested else np.zeros((n_knees, 0))
    X = X[:, None] if X.ndim == 1 else X
    if X.ndim != 2 or X.shape[0] != n_knees or X.shape[1] < int(tested):
        raise ValueError(f"X must be [{n_knees}] or [{n_knees}, k >= 1], got shape {X.shape}")
    cov = np.zeros((n_knees, 0)) if covariates is None else np.asarray(covariates, np.float64)
    cov = cov[:, None] if cov.ndim == 1 else cov
    if cov.ndim != 2 or cov.shape[0] != n_knees:
        raise ValueError(f"covariates must be [{n_knees}] or [{n_knees}, c], got shape {cov.shape}")
    k = X.shape[1]
    names = [f"X column {j}" for j in range(k)] if names is None else list(names)
    p = cov.shape[1] + k + int(bool(intercept))
    if p > ops.MAX_DESIGN_COLUMNS:
        raise ValueError(f"the design has {p} columns ({'the intercept, ' if intercept else ''}{cov.shape[1]} covariates, {k} tested columns); at most "
                         f"{ops.MAX_DESIGN_COLUMNS} are supported")
    named = [(f"covariate {j}", cov[:, j]) for j in range(cov.shape[1])] + list(zip(names, X.T))
    cols = []
    for name, c in named:
        if not np.isfinite(c).all():
            raise ValueError(f"{name} holds a NaN or an infinity: the design must be finite for every knee")
        if (c == c[0]).all():
            raise ValueError(f"{name} is constant over the knees")
        c = c - c.mean() if intercept else c.copy()
        norm = float(np.sqrt((c * c).sum()))
        if not norm > 0.0:
            raise ValueError(f"{name} is constant over the knees")
        cols.append((c, norm))
    Z = ([np.ones(n_knees)] if intercept else []) + [c / s for c, s in cols[:cov.shape[1]]]
    nuisance = np.stack(Z, axis=1) if Z else np.zeros((n_knees, 0))
    design = np.ascontiguousarray(np.concatenate([nuisance] + [(c / s)[:, None] for c, s in cols[cov.shape[1]:]], axis=1))
    unit = design / np.sqrt((design * design).sum(axis=0))[None, :]
    every = (["the intercept"] if intercept else []) + [name for name, _ in named]
    for j in range(p):                                                     # the first column that the ones before it already span
        if n_knees < j + 1 or np.linalg.matrix_rank(unit[:, :j + 1]) < j + 1:
            raise ValueError(f"the design does not have full column rank over the knees: {every[j]} is a combination of the columns before it")
    return np.ascontiguousarray(nuisance), design, np.asarray([s for _, s in cols[cov.shape[1]:]], np.float64)


def _design_columns(x, covariates, intercept: bool, n_knees: int) -> Tuple[np.ndarray, np.ndarray, float]:
    """``_design_matrix`` of ONE regressor, one entry per knee: (nuisance [N, q], design [N, q + 1] with x last, the scale x was divided by)."""
    x = np.asarray(x, np.float64)
    if x.shape != (n_knees,):
        raise ValueError(f"x must hold one entry per knee of the cohort ({n_knees}), got shape {x.shape}")
    nuisance, design, scales = _design_matrix(x, covariates, intercept, n_knees, ["x"])
    return nuisance, design, float(scales[0])


def _index_rows(permutations, make, n_knees: int) -> IndexPermutations:
    perms = make() if permutations is None else permutations
    if not isinstance(perms, IndexPermutations):
        perms = IndexPermutations(np.asarray(perms))
    index = np.atleast_2d(perms.index)
    if index.ndim != 2 or index.shape[1] != n_knees or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"permutations must be integer rows [P, {n_knees}], got {index.dtype} {index.shape}")
    if not np.array_equal(index[0], np.arange(n_knees)):
        raise ValueError("row 0 of the permutations must be the identity")
    if not np.array_equal(np.sort(index, axis=1), np.broadcast_to(np.arange(n_knees), index.shape)):
        raise ValueError("every row of the permutations must be a permutation of 0 .. N - 1")
    return IndexPermutations(np.ascontiguousarray(index, dtype=np.int32), perms.exact)


# ---- vertex-wise design columns (include/oai_hip.h, "Vertex-wise design columns"; csrc/group_regression_vx.hip) ------------------------------
def _is_map(x) -> bool:
    """Is ``x`` one number per (knee, vertex) -- a ``ThicknessCohort`` or a two-dimensional array or tensor -- and not one per knee?"""
    return isinstance(x, ThicknessCohort) or (not isinstance(x, (list, tuple)) and getattr(x, "ndim", 1) == 2)


def _vertex_maps(cohort: ThicknessCohort, maps, name: str) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """The per-vertex columns that ``name`` (``vertex_covariates`` or ``x``) passes, each as (float32 values [N, V], uint8 mask [N, V]) on
    the cohort's GPU in the cohort's row order: a ``ThicknessCohort`` on the same atlas, cartilage and device whose rows are matched BY ID
    as ``paired_test`` matches them, or an [N, V] array or tensor in row order with NaN for a missing entry; or a list of such."""
    if maps is None:
        return []
    N, V, dev = len(cohort), cohort.n_verts, cohort.device
    out = []
    for k, one in enumerate(maps if isinstance(maps, (list, tuple)) else [maps]):
        what = name if not isinstance(maps, (list, tuple)) else f"{name}[{k}]"
        if isinstance(one, ThicknessCohort):
            if one.kind != cohort.kind or one.n_verts != V or one.device != dev:
                raise ValueError(f"{what} must hold the same cartilage of the same atlas on the same GPU as the cohort ({cohort.kind!r}, {V} vertices, "
                                 f"{dev}), got {one.kind!r}, {one.n_verts} vertices, {one.device}")
            where = {id_: i for i, id_ in enumerate(one.ids)}
            if len(where) != len(one) or len(set(cohort.ids)) != N or set(cohort.ids) != set(where):
                raise ValueError(f"{what} needs the same ids as the cohort, each once")
            order = torch.tensor([where[id_] for id_ in cohort.ids], dtype=torch.int64, device=dev)
            out.append((one.values.index_select(0, order), one.mask.index_select(0, order)))
            continue
        if isinstance(one, torch.Tensor):
            if one.device != dev:
                raise ValueError(f"{what} must live on the cohort's GPU ({dev}), got {one.device}")
            vec = one.to(torch.float32)
        else:
            vec = torch.from_numpy(np.ascontiguousarray(np.asarray(one, np.float32))).to(dev)
        if tuple(vec.shape) != (N, V):
            raise ValueError(f"{what} must be a ThicknessCohort or [{N}, {V}] (one row per knee of the cohort, one entry per vertex), got shape "
                             f"{tuple(vec.shape)}")
        ok = ~torch.isnan(vec)
        out.append((torch.where(ok, vec, torch.zeros_like(vec)), ok.to(torch.uint8)))
    return out


def _t_result(cohort: ThicknessCohort, host: dict, shared: dict, perms: IndexPermutations, p: int, scale: float) -> RegressionResult:
    """The ``RegressionResult`` of one download."""
    t, n = host["t"], host["n"]
    dof = n.astype(np.int64) - p
    with np.errstate(invalid="ignore", divide="ignore"):
        partial_r = t / np.sqrt(t * t + dof.astype(np.float64))
    return RegressionResult(kind=cohort.kind, n=n, dof=dof, slope=host["slope"] / scale, partial_r=partial_r, exact=perms.exact, **shared)


# What a statistic of the linear-model tests brings of its own: the batch op and the entry point whose workspace it takes, without and
# with per-vertex columns, and what row 0 also gives (the op's argument for it is that name + "0").
_LINEAR_MODEL_OPS = {"t": ((ops.regression_t, "oai_regression_t"), (ops.regression_vx_t, "oai_regression_vx_t"), "slope"),
                     "f": ((ops.regression_f, "oai_regression_f"), (ops.regression_vx_f, "oai_regression_vx_f"), "coef")}


def _linear_model_test(cohort: ThicknessCohort, what: str, stat: str, X, names, covariates, intercept: bool, n_permutations, cluster_threshold,
                       seed, blocks, permutations, batch, tfce, vertex_covariates=None, x_map=None, groups=None):
    """The one driver of ``regression_test`` (``stat`` "t": the t of the last design column, ``X`` the regressor or, beside ``x_map``,
    None) and of ``f_test`` and ``anova_test`` ("f": the F of the columns of ``X``, jointly; ``names``: ``_design_matrix``'s).
    ``vertex_covariates``, ``x_map``: per-vertex nuisance columns and the per-vertex regressor of interest (``regression_test`` says what
    they are), or None; then the maps stand around the global design and ``n`` / ``dof`` count the complete cases.  ``groups``: (levels,
    the level index of every knee) of ``anova_test`` -- then also the counted means."""
    tfce = _tfce_settings(tfce)
    N, centre = len(cohort), bool(intercept)
    if N < 2:
        raise ValueError(f"{what} needs at least two knees")

    def host_design():
        if stat == "t" and x_map is None:                                  # one regressor: its own shape check, its scale a number
            return _design_columns(X, covariates, centre, N)
        return _design_matrix(X, covariates, centre, N, names)

    vx = vertex_covariates is not None or x_map is not None
    if vx:                 # the maps and the column counts are refused first, the host design after the permutations and the batch
        pg = _n_columns(covariates) + int(centre) + _n_columns(X)          # the global columns of the design
        nuis, interest = _vertex_maps(cohort, vertex_covariates, "vertex_covariates"), _vertex_maps(cohort, x_map, "x")
        if len(interest) > 1:
            raise ValueError("x must be ONE map: one regressor of interest")
        S = len(nuis) + len(interest)
        if S > ops.MAX_VERTEX_COLUMNS:
            raise ValueError(f"vertex_covariates: at most {ops.MAX_VERTEX_COLUMNS} per-vertex columns are supported (x as a map counts), got {S}")
        p = S + pg
        if p > ops.MAX_DESIGN_COLUMNS:
            raise ValueError(f"the design has {p} columns ({pg} global ones and {S} per-vertex ones from vertex_covariates and x); at most "
                             f"{ops.MAX_DESIGN_COLUMNS} are supported")
        row_bytes = N * 8 * (pg + pg * (pg + 1) // 2 + 1)
    else:
        nuisance, design, scales = host_design()
        p = design.shape[1]
        row_bytes = _table_bytes(N, p)
    perms = _index_rows(permutations, lambda: index_permutations(N, n_permutations, seed, blocks), N)
    values, mask = cohort.values, cohort.mask
    V, dev = int(values.shape[1]), values.device
    batches = _Batches(cohort, len(perms), V, dev, cluster_threshold, tfce, batch, row_bytes)
    if vx:                                                                 # in the design's order: nuisance first, the regressor of interest last
        columns, masks = torch.stack([c[0] for c in nuis + interest]), torch.stack([c[1] for c in nuis + interest])
        nuisance, design, scales = host_design()
    index = torch.from_numpy(perms.index).to(dev)
    design_d = torch.from_numpy(design).to(dev) if design.shape[1] else None
    nuisance_d = torch.from_numpy(nuisance).to(dev) if nuisance.shape[1] else None
    if vx:
        prepared = ops.regression_vx_prepare(values, mask, columns, masks, nuisance_d, n_vertex_interest=len(interest), centre=centre)
    else:
        prepared = ops.regression_prepare(values, mask, nuisance_d, centre=centre)
    (tile, entry), first = _LINEAR_MODEL_OPS[stat][int(vx)], _LINEAR_MODEL_OPS[stat][2]
    k = () if stat == "t" else (len(scales),)                              # the F ops take k, and their row 0 gives [k, V]
    out0 = torch.empty((*k, V), dtype=torch.float64, device=dev)
    extras = {first: out0, "n": prepared.n}
    if vx:
        extras["n_dropped"] = prepared.n_dropped
    extras.update(_group_sides(values, mask, groups))
    ws = _lib.workspace(entry, dev, batches.rows, V, N, p, *([S] if vx else []))
    host, shared = batches.run(lambda p0, p1: tile(prepared, design_d, index, p0, p1, *k, workspace=ws, **{first + "0": out0 if p0 == 0 else None}),
                               extras)
    if stat == "t":                                                        # a per-vertex x is not rescaled: slope is per unit of the map
        res = _t_result(cohort, host, shared, perms, p, scales if x_map is None else 1.0)
    else:
        res = _f_result(cohort, host, shared, perms, p, scales, groups)
    if vx:
        res.n_dropped = host["n_dropped"]
    return res


def regression_test(cohort: ThicknessCohort, x, covariates=None, intercept: bool = True, n_permutations: int = 10000,
                    cluster_threshold: Optional[float] = None, seed: int = 0, blocks=None, permutations=None,
                    batch: Optional[int] = None, tfce=None, vertex_covariates=None) -> RegressionResult:
    """How does thickness vary with ``x`` (one entry per knee: KL grade, BMI, years since baseline, or a 0 / 1 dummy), vertex by vertex,
    adjusted for ``covariates`` ([N] or [N, k]: age, a sex dummy, ...) and, with ``intercept``, a constant?  Per vertex the general linear
    model over the knees with a value there, and the t of the coefficient of ``x``; its null distribution comes from Freedman-Lane
    permutation (include/oai_hip.h) with the rows of ``index_permutations(N, n_permutations, seed, blocks)``, or of ``permutations`` (an
    ``IndexPermutations`` or int rows [P, N], row 0 the identity).  At most six design columns in all.  The columns are centred (with an
    intercept) and scaled to unit length on the host, which changes neither t nor the p-values; ``slope`` is given per unit of the ``x``
    that was passed.  ``cluster_threshold``, ``batch``, ``tfce``: as in ``two_sample_test`` (default batch: ``regression_batch``).

    ``vertex_covariates``: one or two MAPS to adjust for at every vertex -- baseline thickness at the same vertex above all, without
    which a rate of change regresses to the mean (include/oai_hip.h, "Vertex-wise design columns"; csrc/group_regression_vx.hip;
    tests/vertex_regression_ref.py).  A ``ThicknessCohort`` on the same atlas, cartilage and GPU whose rows are matched to the cohort's BY
    ID (the same ids, each once), an [N, V] array or tensor in row order with NaN for a missing entry, or a list of at most two of these.
    ``x`` may itself be such a map: the regressor of interest is then per vertex and ``slope`` is per unit of the map.  At most two
    per-vertex columns and six columns in all.  The analysis is complete-case per vertex: a knee counts where its value AND its
    covariates are there; ``n`` and ``dof`` count those, and ``n_dropped`` (None without per-vertex columns) the knees with a value that
    a missing covariate dropped.  The observed statistic is the exact complete-case fit; within the null distribution a permuted design
    row whose covariate is missing stands on the complete-case mean.  Per-vertex columns are centred (with an intercept) on the device and
    not rescaled.  The coefficient of a per-vertex NUISANCE column is not returned: pass it as ``x`` to get it.  None: the test runs as
    it always has."""
    x, x_map = (None, x) if _is_map(x) else (x, None)                          # beside a map every global column is nuisance
    return _linear_model_test(cohort, "regression_test", "t", x, None, covariates, intercept, n_permutations, cluster_threshold, seed, blocks,
                              permutations, batch, tfce, vertex_covariates=vertex_covariates, x_map=x_map)


# ---- one-stage models of clustered rows (include/oai_hip.h, "Cluster-robust regression"; csrc/cluster_robust.hip) ----------------------------
@dataclass
class MarginalResult(_SurfaceResult):
    """``t`` float64 [V]: the cluster-robust (sandwich, CR1) t of the regressor's coefficient in the ordinary least squares fit over all
    rows (NaN where no t exists: fewer than two clusters with a value, too few rows, a design that loses its rank among them, no
    residual variation); ``slope`` per unit of ``x`` and ``se`` its sandwich standard error; ``n`` the valid rows and ``n_clusters`` the
    clusters with a valid row (G) per vertex; ``dof`` = G - 1, the degrees of freedom a t table would be read at (the p-values here come
    from the bootstrap, not from a table); ``p_uncorrected``, ``p_fwer``, ``max_abs`` and the cluster and TFCE fields as in
    ``PermutationResult``, over the ``n_bootstrap`` sign vectors of the wild cluster bootstrap (``exact``: all 2^S of them)."""
    kind: str
    t: np.ndarray
    slope: np.ndarray
    se: np.ndarray
    n: np.ndarray
    n_clusters: np.ndarray
    dof: np.ndarray
    p_uncorrected: np.ndarray
    p_fwer: np.ndarray
    max_abs: np.ndarray
    n_bootstrap: int
    exact: bool

    IMAGES = ("t", "slope", "se", "p_fwer", "p_uncorrected", "n", "n_clusters", "cluster_label", "tfce", "p_tfce")


def cluster_rows(labels) -> Tuple[List[object], np.ndarray, np.ndarray]:
    """Rows grouped by cluster: (the clusters in order of first appearance, ``order`` int64 [N] -- the rows in CLUSTER-MAJOR order, input
    order within a cluster -- and ``offsets`` int32 [S+1]: cluster s owns ``order[offsets[s] : offsets[s+1]]``)."""
    index: dict = {}
    owner = np.asarray([index.setdefault(lab, len(index)) for lab in labels], np.int64)
    order = np.argsort(owner, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(index)))]).astype(np.int32)
    return list(index), order, offsets


def marginal_test(cohort_or_visits, x, covariates=None, clusters=None, intercept: bool = True, n_bootstrap: int = 10000,
                  cluster_threshold: Optional[float] = None, tfce=None, seed: int = 0, flips=None, batch: Optional[int] = None) -> MarginalResult:
    """How does thickness vary with ``x`` over rows that come in CLUSTERS -- the visits of a subject (a ``LongitudinalCohort``: the
    clusters default to its subjects) or both knees of a subject (a ``ThicknessCohort`` with ``clusters``, one hashable per row: the
    subject of each knee)?  The one-stage marginal model (include/oai_hip.h, "Cluster-robust regression"): ordinary least squares over
    all rows with a value at the vertex, the cluster-robust sandwich variance (CR1) and its t, and a null distribution from the restricted
    wild cluster bootstrap -- ``sign_flips(S, n_bootstrap, seed)`` over the S clusters (all 2^S when there are at most ``n_bootstrap``),
    or ``flips``, which takes what ``permutations`` takes in ``paired_test`` with one bit per cluster in order of first appearance.
    ``x`` and ``covariates`` ([N] or [N, k]) are per ROW, in the order the rows were added, so a covariate may vary within a subject
    (years, BMI or pain at the visit; ``visits.years``, ``visits.per_row``); a constant or collinear column is refused by name.  At most
    six design columns.  ``cluster_threshold``, ``tfce``, ``batch``: as in ``two_sample_test``.

    Limits: one regressor of interest (no joint Wald F); CR1 only (no CR2 / CR3 or SwE small-sample corrections); Rademacher weights
    only, so with S <= 11 clusters the null has at most 2^S points; the wild bootstrap is LIBERAL with few clusters (about 8 % rejections
    at a nominal 5 % with 24 clusters in a simulation on the restatement) and no significance level is built in; no subject fixed effects
    or within-subject centring; no per-vertex design columns; no rank wrapper; missingness stays attached to the row; the cluster block
    takes (2 p + 1) * S * V * 8 bytes on the device."""
    tfce = _tfce_settings(tfce)
    if isinstance(cohort_or_visits, LongitudinalCohort):
        cohort = cohort_or_visits.rows
        labels = list(cohort_or_visits._subject) if clusters is None else list(clusters)
    else:
        cohort = cohort_or_visits
        if clusters is None:
            raise ValueError("marginal_test on a ThicknessCohort needs clusters=: one hashable per row (the subject of each knee)")
        labels = list(clusters)
    N = len(cohort)
    if len(labels) != N:
        raise ValueError(f"clusters must hold one label per row of the cohort ({N}), got {len(labels)}")
    names, order, offsets = cluster_rows(labels)
    S = len(names)
    if S < 2:
        raise ValueError(f"marginal_test needs at least two clusters, got {S}")
    _, design, scale = _design_columns(x, covariates, bool(intercept), N)
    if flips is not None and not isinstance(flips, Permutations) and np.asarray(flips).dtype == bool and np.atleast_2d(flips).shape[1] != S:
        raise ValueError(f"the flips must hold one bit per cluster ({S}), got bool rows of {np.atleast_2d(flips).shape[1]}")
    perms = _permutations(flips, lambda: sign_flips(S, n_bootstrap, seed), S)
    if perms.n_knees != S or perms.bits.ndim != 2 or perms.bits.shape[1] != (S + 31) // 32:
        raise ValueError(f"the flips must hold one bit per cluster ({S}), got rows for {perms.n_knees} in {perms.bits.shape}")
    if perms.rows()[0].any():
        raise ValueError("row 0 of the flips must flip nothing")
    P, V, dev = len(perms), cohort.n_verts, cohort.device
    pick = torch.from_numpy(order).to(dev)
    values, mask = cohort.values.index_select(0, pick), cohort.mask.index_select(0, pick)
    batches = _Batches(cohort, P, V, dev, cluster_threshold, tfce, batch)
    bits = torch.from_numpy(np.ascontiguousarray(perms.bits).view(np.int32)).to(dev)
    prepared = ops.cluster_prepare(values, mask, torch.from_numpy(np.ascontiguousarray(design[order])).to(dev), torch.from_numpy(offsets).to(dev),
                                   centre=bool(intercept))
    slope0, se0 = (torch.empty(V, dtype=torch.float64, device=dev) for _ in range(2))
    ws = _lib.workspace("oai_cluster_t", dev, batches.rows, V)
    first = lambda p0: dict(slope0=slope0, se0=se0) if p0 == 0 else {}
    host, shared = batches.run(lambda p0, p1: ops.cluster_t(prepared, bits, p0, p1, workspace=ws, **first(p0)),
                               {"slope": slope0, "se": se0, "n": prepared.n, "n_clusters": prepared.G})
    shared["n_bootstrap"] = shared.pop("n_permutations")
    return MarginalResult(kind=cohort.kind, slope=host["slope"] / scale, se=host["se"] / scale, n=host["n"], n_clusters=host["n_clusters"],
                          dof=host["n_clusters"].astype(np.int64) - 1, exact=perms.exact, **shared)


# ---- F tests ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class FResult(_SurfaceResult):
    """``f`` float64 [V]: the F of the columns tested jointly, given the covariates (NaN where no F exists: too few knees with a value, a
    design that loses its rank among them -- a level of the factor without a knee there --, no residual variance); ``n`` the knees with a
    value, ``dof1`` = k, the number of columns tested, and ``dof2`` = n - p per vertex; ``coefficients`` float64 [k, V] in mm per unit of
    the column as passed -- of ``anova_test``: the level's adjusted difference from the first level; ``partial_eta2`` = k f / (k f + dof2),
    the share of the variance left by the covariates that the tested columns explain; ``p_uncorrected`` = share of permutations with an F
    at least the observed at that vertex, ``p_fwer`` = share of permutations whose maximal F over the surface is at least the observed F
    at that vertex (both NaN where f is); ``max_f`` the null distribution of the surface maximum, entry 0 observed.  ``levels`` (the sorted
    labels), ``group_n`` int32 [G, V] and ``group_mean`` float64 [G, V] (the counted, unadjusted mean of each level's knees per vertex) are
    filled by ``anova_test`` and None from ``f_test``.  The cluster and TFCE fields are as in ``PermutationResult``, with two differences that
    follow from F >= 0: ``cluster_threshold`` is an F value and every cluster has sign +1; and TFCE is applied to the F tile AS IT IS.  F
    scales like t squared, so the height exponent H = 1 on F weighs height roughly as H = 2 does on |t|, and ``TFCE.dh`` is a step in units
    of F; ``tfce_clipped`` counts the permutations with an F beyond ``max_steps * dh``.  Neither is adjusted behind the caller's back:
    ``tfce=True`` means the same ``TFCE()`` as in the other tests."""
    kind: str
    f: np.ndarray
    n: np.ndarray
    dof1: int
    dof2: np.ndarray
    coefficients: np.ndarray
    partial_eta2: np.ndarray
    p_uncorrected: np.ndarray
    p_fwer: np.ndarray
    max_f: np.ndarray
    n_permutations: int
    exact: bool
    levels: Optional[np.ndarray] = None
    group_n: Optional[np.ndarray] = None
    group_mean: Optional[np.ndarray] = None

    IMAGES = ("f", "partial_eta2", "p_fwer", "p_uncorrected", "n", "cluster_label", "tfce", "p_tfce")
    n_dropped = None        # as in ``RegressionResult``: set with ``vertex_covariates``, when ``n`` and ``dof2`` count the complete cases


def _group_sides(values: torch.Tensor, mask: torch.Tensor, groups) -> dict:
    """The descriptive side of ``anova_test``: n and mean of every level, per vertex, as device tensors to download with the rest."""
    sides = {}
    if groups is not None:
        for g in range(len(groups[0])):
            idx = torch.from_numpy(np.nonzero(groups[1] == g)[0]).to(values.device)
            prep = ops.group_prepare(values.index_select(0, idx), mask.index_select(0, idx))
            sides.update({f"n{g}": prep.n, f"mean{g}": prep.mean})
    return sides


def _f_result(cohort: ThicknessCohort, host: dict, shared: dict, perms: IndexPermutations, p: int, scales: np.ndarray, groups) -> FResult:
    """The ``FResult`` of one download."""
    f, n, k = shared.pop("t"), host["n"], len(scales)
    dof2 = n.astype(np.int64) - p
    with np.errstate(invalid="ignore", divide="ignore"):
        partial_eta2 = (k * f) / (k * f + dof2.astype(np.float64))
    described = {}
    if groups is not None:
        G = len(groups[0])
        described = dict(levels=groups[0], group_n=np.stack([host[f"n{g}"] for g in range(G)]), group_mean=np.stack([host[f"mean{g}"] for g in range(G)]))
    return FResult(kind=cohort.kind, f=f, n=n, dof1=k, dof2=dof2, coefficients=host["coef"] / scales[:, None], partial_eta2=partial_eta2,
                   max_f=shared.pop("max_abs"), exact=perms.exact, **described, **shared)


def f_test(cohort: ThicknessCohort, X, covariates=None, intercept: bool = True, n_permutations: int = 10000,
           cluster_threshold: Optional[float] = None, seed: int = 0, blocks=None, permutations=None, batch: Optional[int] = None,
           tfce=None, vertex_covariates=None) -> FResult:
    """Do the columns of ``X`` ([N] or [N, k]: the dummies of a factor, an interaction with its main effect, a linear and a quadratic
    term) explain thickness JOINTLY, vertex by vertex, adjusted for ``covariates`` ([N] or [N, c]) and, with ``intercept``, a constant?  Per
    vertex the general linear model over the knees with a value there and the F of the k columns given the others (include/oai_hip.h,
    "Cohort F test"; csrc/group_regression.hip; tests/group_f_ref.py); its null distribution comes from Freedman-Lane permutation with the
    rows of ``index_permutations(N, n_permutations, seed, blocks)``, or of ``permutations``, as in ``regression_test``.  At most six design
    columns in all.  The columns are centred (with an intercept) and scaled to unit length on the host, which changes neither F nor the
    p-values; ``coefficients`` are given per unit of the columns that were passed.  Refused before anything is launched: a NaN or an
    infinity, a constant column, more than six columns, a design without full column rank -- the message names the column.
    ``cluster_threshold`` is an F value; ``batch`` as in ``regression_test``; ``tfce``: True or a ``TFCE``, applied to F as it is -- F scales
    like t squared, so H = 1 on F weighs height roughly as H = 2 does on |t|, and ``dh`` and ``max_steps * dh`` are in units of F
    (``FResult`` says more).  With k = 1, F is the square of ``regression_test``'s t and the p-values are those of its two-sided test.
    ``vertex_covariates``: one or two maps to adjust for at every vertex, as in ``regression_test``, which says what they are and what
    ``n``, ``dof2`` and ``n_dropped`` then count; the tested columns themselves are one number per knee (a map as ``X`` is refused: test
    it with ``regression_test(cohort, x=map)``)."""
    if isinstance(X, ThicknessCohort) or (_is_map(X) and X.shape[-1] > ops.MAX_DESIGN_COLUMNS and X.shape[-1] == cohort.n_verts):
        raise ValueError("X must hold one entry per knee and column: a map (one entry per knee and vertex) is tested with regression_test(cohort, x=map)")
    return _linear_model_test(cohort, "f_test", "f", X, None, covariates, intercept, n_permutations, cluster_threshold, seed, blocks, permutations,
                              batch, tfce, vertex_covariates=vertex_covariates)


def _anova_levels(groups, n_knees: int, n_covariates: int) -> Tuple[np.ndarray, np.ndarray]:
    """(the sorted labels, the level index of every knee); refuses what ``anova_test`` does."""
    g = np.asarray(groups)
    if g.shape != (n_knees,):
        raise ValueError(f"groups must hold one label per knee of the cohort ({n_knees}), got shape {g.shape}")
    if g.dtype.kind not in "iuf" or (g.dtype.kind == "f" and not (np.isfinite(g).all() and (g == np.rint(g)).all())):
        raise ValueError(f"groups must be integer labels, got {g.dtype}" + (" with values that are not whole numbers" if g.dtype.kind == "f" else ""))
    levels, where, count = np.unique(g.astype(np.int64), return_inverse=True, return_counts=True)
    if len(levels) < 2:
        raise ValueError(f"groups holds a single level ({int(levels[0])}): an analysis of variance needs at least two")
    p = 1 + n_covariates + len(levels) - 1
    if len(levels) > ops.MAX_DESIGN_COLUMNS or p > ops.MAX_DESIGN_COLUMNS:
        raise ValueError(f"{len(levels)} levels and {n_covariates} covariates make a design of {p} columns (the intercept, the covariates, a dummy "
                         f"for every level after the first); at most {ops.MAX_DESIGN_COLUMNS} are supported")
    if count.min() < 2:
        raise ValueError(f"level {int(levels[count.argmin()])} has {int(count.min())} knee: every level needs at least two")
    return levels, where.reshape(-1)


def anova_test(cohort: ThicknessCohort, groups, covariates=None, n_permutations: int = 10000, cluster_threshold: Optional[float] = None,
               seed: int = 0, blocks=None, permutations=None, batch: Optional[int] = None, tfce=None, vertex_covariates=None) -> FResult:
    """Does thickness differ ACROSS the levels of a factor (``groups``: an integer label per knee with 2 to 6 distinct levels -- KL grade,
    site, treatment arm), vertex by vertex, adjusted for ``covariates``?  One-way analysis of (co)variance: the design is an intercept, the
    covariates and a 0 / 1 dummy for every level after the smallest one, and the dummies are tested jointly as in ``f_test``, whose other
    arguments these are.  The six-column limit holds: levels - 1 + covariates + 1 <= 6.  Every level needs at least two knees.
    ``coefficients[j]`` is the adjusted difference of level ``levels[j + 1]`` from level ``levels[0]``; ``group_n`` and ``group_mean`` are the
    counted, unadjusted figures of every level.  Which level is the first changes the coefficients and not F.  ``vertex_covariates``: as in
    ``f_test``; the maps count towards the six columns."""
    if _is_map(groups):
        raise ValueError("groups must hold one label per knee: a map (one entry per knee and vertex) is tested with regression_test(cohort, x=map)")
    levels, where = _anova_levels(groups, len(cohort), _n_columns(covariates))
    dummies = np.stack([(where == g).astype(np.float64) for g in range(1, len(levels))], axis=1)
    names = [f"the dummy of level {int(lab)}" for lab in levels[1:]]
    return _linear_model_test(cohort, "anova_test", "f", dummies, names, covariates, True, n_permutations, cluster_threshold, seed, blocks,
                              permutations, batch, tfce, vertex_covariates=vertex_covariates, groups=(levels, where))


# ---- normative deviation ---------------------------------------------------------------------------------------------------------------
_DEVIATION_BYTES = 8 + 8              # per (knee, vertex) of a batch: the z tile and oai_graph_clusters_workspace_bytes
_MODEL_ARRAYS = ("gamma", "L", "rss", "n", "ok")


def _rank_p(stat, reference, member: bool) -> np.ndarray:
    """The family-wise p of each knee's statistic against the reference knees' own leave-one-out statistics:
    (1 + #{reference knees j: stat_j >= stat}) / (N' + 1).  For a ``member`` of the reference, itself is left out of the count (it is one of
    the j, and stat_j >= stat holds for it) and N' = N - 1; for any other knee N' = N.  The smallest possible p is 1 / (N' + 1)."""
    ref = np.sort(np.asarray(reference))
    ge = len(ref) - np.searchsorted(ref, np.asarray(stat), side="left")
    return ge / float(len(ref)) if member else (1.0 + ge) / float(len(ref) + 1)


def _normative_design(covariates, intercept: bool, n_knees: int, names: Optional[Sequence[str]] = None):
    """(design [N, p], means [c], scales [c], names) of a reference cohort: the intercept (if any) first, then every covariate column less
    its mean over the reference (with an intercept) and divided by its length, as ``_design_matrix`` makes them -- whose refusals, by
    name and before anything is launched, these are: a NaN or an infinity, a constant or a collinear column, more than six columns."""
    if covariates is None or np.size(covariates) == 0:
        if not intercept:
            raise ValueError("a model without covariates needs the intercept: there is no column left")
        return np.ones((n_knees, 1)), np.zeros(0), np.ones(0), []
    cov = np.asarray(covariates, np.float64)
    cov = cov[:, None] if cov.ndim == 1 else cov
    if cov.ndim != 2 or cov.shape[0] != n_knees:
        raise ValueError(f"covariates must be [{n_knees}] or [{n_knees}, c], got shape {cov.shape}")
    names = [f"covariate {j}" for j in range(cov.shape[1])] if names is None else [str(n) for n in names]
    if len(names) != cov.shape[1]:
        raise ValueError(f"names must hold one entry per covariate column ({cov.shape[1]}), got {len(names)}")
    _, _, scales = _design_matrix(cov, None, intercept, n_knees, names)
    means = np.array([cov[:, j].mean() for j in range(cov.shape[1])]) if intercept else np.zeros(cov.shape[1])
    return _design_rows(cov, intercept, means, scales), means, scales, names


def _design_rows(cov: np.ndarray, intercept: bool, means: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """[M, p]: the design rows of knees with the covariates ``cov`` [M, c], centred and scaled as the reference's columns were."""
    cols = ([np.ones(cov.shape[0])] if intercept else []) + [(cov[:, j] - means[j]) / scales[j] for j in range(cov.shape[1])]
    return np.ascontiguousarray(np.stack(cols, axis=1))


@dataclass
class DeviationResult:
    """One entry per knee (``ids``), scored against a ``NormativeModel`` at ``z_threshold``; ``loo``: the knees are the model's own members,
    each scored as if the model had been fitted without it.  ``max_abs`` = max |z| over the surface at vertex ``max_vertex`` (-1: the knee
    has no score anywhere), ``min_z``, ``max_z``; ``n_valid`` the vertices with a score; ``n_below`` / ``area_below_mm2`` the vertex count
    and atlas area of {z < -z_threshold} -- abnormally thin --, ``n_above`` / ``area_above_mm2`` of {z > z_threshold}; ``max_extent`` the
    vertex count of the largest connected cluster of either set.  ``dof`` int64 [V]: the degrees of freedom of z per vertex (n - p, or
    n - p - 1 for members).  The family-wise per-knee p-values ``p_max``, ``p_extent`` and ``p_area_below`` are ranks of ``max_abs``,
    ``max_extent`` and the area below among the reference knees' own leave-one-out statistics (``_rank_p``): is this knee's worst place,
    largest cluster, thin area more than a healthy knee shows SOMEWHERE on its surface?  No significance level is built in.  With
    ``return_maps``: ``z`` and ``diff_mm`` float64 [M, V] (NaN where there is no score) and ``p_uncorrected``, the two-sided Student t
    p of z at ``dof``, vertex by vertex."""
    kind: str
    ids: List[object]
    loo: bool
    z_threshold: float
    n_valid: np.ndarray
    max_abs: np.ndarray
    max_vertex: np.ndarray
    min_z: np.ndarray
    max_z: np.ndarray
    n_below: np.ndarray
    n_above: np.ndarray
    area_below_mm2: np.ndarray
    area_above_mm2: np.ndarray
    max_extent: np.ndarray
    dof: np.ndarray
    p_max: np.ndarray
    p_extent: np.ndarray
    p_area_below: np.ndarray
    z: Optional[np.ndarray] = None
    diff_mm: Optional[np.ndarray] = None
    p_uncorrected: Optional[np.ndarray] = None
    model: Optional["NormativeModel"] = field(default=None, repr=False, compare=False)

    IMAGES = ("z", "diff_mm", "p_uncorrected")

    def __len__(self) -> int:
        return len(self.ids)

    def _map(self, what: str, knee: int) -> np.ndarray:
        if what not in self.IMAGES:
            raise ValueError(f"no image of {what!r}")
        if getattr(self, what) is None:
            raise ValueError("the knees were scored without return_maps")
        if not 0 <= int(knee) < len(self):
            raise ValueError(f"knee must be 0 .. {len(self) - 1}, got {knee!r}")
        return getattr(self, what)[int(knee)]

    def image(self, atlas, what: str = "z", knee: int = 0):
        """``atlas.image`` of knee ``knee``'s "z", "diff_mm" or "p_uncorrected" map (float32 [H, W], NaN off the surface)."""
        return atlas.image(np.asarray(self._map(what, knee), np.float32), self.kind)

    def clusters(self, knee: int = 0) -> List[Cluster]:
        """The connected clusters of {z < -z_threshold} and {z > z_threshold} of knee ``knee`` in ascending label, from a one-row
        ``ops.graph_clusters`` call; ``p_cluster``: the rank of the extent among the reference's largest leave-one-out clusters."""
        z = self._map("z", knee)
        model = self.model
        offsets, neighbours = model.surface.surface_graph()
        _, label, size = ops.graph_clusters(torch.from_numpy(np.ascontiguousarray(z[None, :])).to(model.device), offsets, neighbours,
                                            self.z_threshold, return_labels=True)
        label, size = _download([label, size])
        area, reference = model.surface.vertex_areas(), model.reference(self.z_threshold)["max_extent"]
        found = []
        for lab in np.unique(label[label >= 0]):
            members = np.nonzero(label == lab)[0]
            found.append(Cluster(int(lab), 1 if z[lab] > 0 else -1, int(size[lab]), float(np.cumsum(area[members])[-1]),
                                 float(_rank_p(int(size[lab]), reference, self.loo))))
        return found


class NormativeModel:
    """Where is ONE knee abnormally thin for its age, sex and BMI?  A linear model of thickness on covariates, fitted per vertex on a
    reference cohort (include/oai_hip.h, "Normative deviation"; csrc/normative.hip; tests/normative_ref.py), against which single knees are
    scored: z = the knee's residual over the standard error of a new observation, which holds the residual variance of the reference AND
    the uncertainty of the fitted mean at the knee's covariates.  ``deviation`` scores knees that are not in the fit, ``loo`` the members
    themselves, each against the fit without it (the externally studentised residual, in closed form).  Fitted on the rate maps of
    non-progressors (``LongitudinalCohort.change("rate")``), the same model gives per-knee progressor maps.

    Limits.  At most six design columns, the intercept among them.  A knee without a value at a vertex has no score there.  Reference
    knees are scored against N - 1 others and a new knee against N, so their statistics are t variables with one degree of freedom less
    and exchangeable with the new knee's only approximately.  The smallest possible p is 1 / (N + 1).  No TFCE of the z tile, no float32 z."""

    def __init__(self, surface: ThicknessCohort, block: "ops.NormativeFit", n_knees: int, intercept: bool, names, means, scales):
        self.surface, self.block, self.n_knees, self.intercept = surface, block, int(n_knees), bool(intercept)
        self.names, self.means, self.scales = list(names), np.asarray(means, np.float64), np.asarray(scales, np.float64)
        self.atlas, self.kind, self.device, self.n_verts = surface.atlas, surface.kind, surface.device, surface.n_verts
        self.n_columns = int(block.n_columns)
        self.cohort: Optional[ThicknessCohort] = None          # the reference itself; None on a model that was loaded
        self.design: Optional[np.ndarray] = None               # its design [N, p]
        self._reference: dict = {}                             # z_threshold -> the reference's own leave-one-out statistics
        self._weights: Optional[torch.Tensor] = None

    @classmethod
    def fit(cls, cohort: ThicknessCohort, covariates=None, intercept: bool = True, names: Optional[Sequence[str]] = None) -> "NormativeModel":
        """The model of the reference ``cohort`` on ``covariates`` ([N] or [N, c]; None: the mean alone) and, with ``intercept``, a constant.
        Every covariate column is centred on its mean over the reference and scaled to unit length; the means and scales are kept for the
        knees to come.  Refused by name before anything is launched: a NaN or an infinity, a constant or a collinear column (``names``: what
        the columns are called), more than six columns, fewer than p + 2 knees."""
        N = len(cohort)
        design, means, scales, names = _normative_design(covariates, bool(intercept), N, names)
        p = design.shape[1]
        if N < p + 2:
            raise ValueError(f"a reference of {N} knees is too small for {p} design columns: a leave-one-out score needs at least p + 2 = {p + 2}")
        block = ops.normative_fit(cohort.values, torch.from_numpy(design).to(cohort.device), cohort.mask)
        model = cls(cohort, block, N, bool(intercept), names, means, scales)
        model.cohort, model.design = cohort, design
        return model

    # -- the host side of a model ---------------------------------------------------------------------------------------------------------
    def rows(self, covariates, n_rows: int) -> np.ndarray:
        """float64 [M, p]: the design rows of ``n_rows`` knees with ``covariates`` ([M, c]; [c] or a scalar for one knee; None for a model
        without covariates), centred and scaled as the reference's were."""
        c = len(self.means)
        cov = np.zeros((n_rows, 0)) if covariates is None else np.asarray(covariates, np.float64)
        if cov.ndim < 2:
            cov = cov.reshape(n_rows, -1) if cov.size == n_rows * c and c > 0 else cov.reshape(1, -1)
        if cov.shape != (n_rows, c):
            raise ValueError(f"covariates must hold the model's {c} columns ({', '.join(self.names) or 'none'}) for each of the {n_rows} knees, "
                             f"got shape {np.shape(covariates) if covariates is not None else None}")
        if not np.isfinite(cov).all():
            raise ValueError("covariates hold a NaN or an infinity")
        return _design_rows(cov, self.intercept, self.means, self.scales)

    def state(self) -> dict:
        """What ``save`` writes, as host arrays: the model block's ``gamma``, ``L``, ``rss``, ``n``, ``ok``; ``means``, ``scales``, ``names``,
        ``intercept``, ``kind``, ``n_knees``; and the reference's leave-one-out statistics at every threshold computed so far."""
        host = dict(zip(_MODEL_ARRAYS, _download([getattr(self.block, name) for name in _MODEL_ARRAYS])))
        z0 = sorted(self._reference)
        host.update(means=self.means, scales=self.scales, names=np.asarray(self.names, dtype=np.str_), intercept=np.asarray(self.intercept),
                    kind=np.asarray(self.kind), n_knees=np.asarray(self.n_knees, np.int64), ref_z_threshold=np.asarray(z0, np.float64))
        for name, dtype in (("max_abs", np.float64), ("max_extent", np.int32), ("area_below", np.int64)):
            host["ref_" + name] = np.asarray([self._reference[t][name] for t in z0], dtype).reshape(len(z0), self.n_knees)
        return host

    @staticmethod
    def write_state(path, state: dict) -> None:
        with open(path, "wb") as f:
            np.savez(f, **state)

    @staticmethod
    def read_state(path) -> dict:
        with np.load(path, allow_pickle=False) as f:
            return {name: f[name] for name in f.files}

    def save(self, path, z_thresholds: Sequence[float] = (2.0,)) -> None:
        """Write the model as one ``.npz``: everything ``deviation`` needs for new knees -- the per-vertex fit, the centring of the
        covariates and the reference's own leave-one-out statistics at ``z_thresholds`` (and at every threshold used so far) -- without the
        reference's thickness maps, so that a model built once from a healthy cohort can be shipped."""
        if self.cohort is not None:
            for t in z_thresholds:
                self.reference(t)
        self.write_state(path, self.state())

    @classmethod
    def load(cls, path, atlas) -> "NormativeModel":
        """The model that ``save`` wrote, on ``atlas`` (whose inner mesh of the model's cartilage must have the model's vertices).  It scores
        new knees at the thresholds it was saved with; ``loo`` needs the reference and is not available."""
        s = cls.read_state(path)
        kind = str(s["kind"])
        surface = ThicknessCohort(atlas, kind)
        p, V = int(s["gamma"].shape[0]), int(s["gamma"].shape[1])
        if V != surface.n_verts:
            raise ValueError(f"the model has {V} vertices, the atlas' {kind} inner mesh {surface.n_verts}")
        block = ops.normative_block(V, p, surface.device)
        for name in _MODEL_ARRAYS:
            getattr(block, name).copy_(torch.from_numpy(np.ascontiguousarray(s[name])))
        model = cls(surface, block, int(s["n_knees"]), bool(s["intercept"]), [str(n) for n in s["names"]], s["means"], s["scales"])
        for k, t in enumerate(s["ref_z_threshold"].tolist()):
            model._reference[float(t)] = {name: s["ref_" + name][k] for name in ("max_abs", "max_extent", "area_below")}
        return model

    def predict(self, covariates=None, n_rows: int = 1) -> np.ndarray:
        """float64 [M, V]: the expected map in mm of knees with ``covariates`` ([M, c]; M = ``n_rows`` without covariates), NaN where the
        model has no fit."""
        M = int(n_rows) if covariates is None or np.ndim(covariates) < 2 else int(np.shape(covariates)[0])
        gamma, ok = _download([self.block.gamma, self.block.ok])
        return np.where(ok[None, :] != 0, self.rows(covariates, M) @ gamma, np.nan)

    # -- scoring ----------------------------------------------------------------------------------------------------------------------------
    def _area_weights(self) -> torch.Tensor:
        if self._weights is None:
            self._weights = torch.from_numpy(tfce_weights(self.surface.vertex_areas())).to(self.device)
        return self._weights

    def _score(self, values: torch.Tensor, mask: torch.Tensor, design: np.ndarray, loo: bool, z_threshold: float, return_maps: bool) -> dict:
        """The device side of both scorings, in batches of rows within ``WORKSPACE_BUDGET``: score, summary, clusters; ONE download."""
        if not float(z_threshold) > 0.0:
            raise ValueError(f"z_threshold must be > 0, got {z_threshold!r}")
        M, V, dev = int(values.shape[0]), self.n_verts, self.device
        offsets, neighbours = self.surface.surface_graph()
        weights, design_d = self._area_weights(), torch.from_numpy(design).to(dev)
        rows = int(max(1, min(M, WORKSPACE_BUDGET // (V * _DEVIATION_BYTES))))
        # with maps the tiles of all batches lie behind one another in one buffer, which is the z map; 256 bytes more: a tile's size is rounded up
        buffer = torch.empty((M if return_maps else rows) * V * 8 + 256, dtype=torch.uint8, device=dev)
        diff = torch.empty((M, V), dtype=torch.float64, device=dev) if return_maps else None
        extent = torch.empty(M, dtype=torch.int32, device=dev)
        stats, counts = [], []
        with torch.cuda.device(dev):
            for r0 in range(0, M, rows):
                r1 = min(r0 + rows, M)
                tile = ops.normative_score(self.block, values[r0:r1], design_d[r0:r1], mask[r0:r1], loo=loo,
                                           workspace=buffer[r0 * V * 8:] if return_maps else buffer, diff=diff[r0:r1] if return_maps else None)
                s, c = ops.deviation_summary(tile, z_threshold, weights)
                stats.append(s)
                counts.append(c)
                ops.graph_clusters(tile, offsets, neighbours, float(z_threshold), max_extent=extent[r0:r1])
            bring = {"stats": torch.cat(stats), "counts": torch.cat(counts), "max_extent": extent, "n": self.block.n}
            if return_maps:
                bring.update(z=buffer[:M * V * 8].view(torch.float64).reshape(M, V), diff_mm=diff)
            return dict(zip(bring, _download(list(bring.values()))))

    def reference(self, z_threshold: float = 2.0) -> dict:
        """The reference knees' own leave-one-out statistics at ``z_threshold`` -- ``max_abs`` float64, ``max_extent`` int32 and
        ``area_below`` int64 (units of 2^-20 mm^2), [N] each -- which every p-value is a rank among; computed once and kept."""
        key = float(z_threshold)
        if key not in self._reference:
            if self.cohort is None:
                raise ValueError(f"the model was saved without the reference's statistics at z_threshold = {key}: it has them at "
                                 f"{sorted(self._reference)}")
            host = self._score(self.cohort.values, self.cohort.mask, self.design, True, key, False)
            self._reference[key] = {"max_abs": host["stats"][:, 0].copy(), "max_extent": host["max_extent"], "area_below": host["counts"][:, 3].copy(),
                                    "host": host}
        return self._reference[key]

    def _result(self, host: dict, ids, loo: bool, z_threshold: float) -> DeviationResult:
        ref = self.reference(z_threshold)
        stats, counts = host["stats"], host["counts"]
        dof = host["n"].astype(np.int64) - self.n_columns - (1 if loo else 0)
        maps = {}
        if "z" in host:
            from scipy import stats as scipy_stats
            with np.errstate(invalid="ignore"):
                p_unc = 2.0 * scipy_stats.t.sf(np.abs(host["z"]), np.maximum(dof, 1)[None, :])
            maps = dict(z=host["z"], diff_mm=host["diff_mm"], p_uncorrected=np.where(np.isnan(host["z"]), np.nan, p_unc))
        return DeviationResult(kind=self.kind, ids=list(ids), loo=loo, z_threshold=float(z_threshold), n_valid=counts[:, 0], max_abs=stats[:, 0],
                               max_vertex=counts[:, 1], min_z=stats[:, 1], max_z=stats[:, 2], n_below=counts[:, 2], n_above=counts[:, 4],
                               area_below_mm2=counts[:, 3] * _TFCE_AREA_UNIT, area_above_mm2=counts[:, 5] * _TFCE_AREA_UNIT,
                               max_extent=host["max_extent"], dof=dof, p_max=_rank_p(stats[:, 0], ref["max_abs"], loo),
                               p_extent=_rank_p(host["max_extent"], ref["max_extent"], loo),
                               p_area_below=_rank_p(counts[:, 3], ref["area_below"], loo), model=self, **maps)

    def loo(self, z_threshold: float = 2.0, return_maps: bool = False) -> DeviationResult:
        """The reference's own knees, each scored against the fit WITHOUT it -- the externally studentised residual, which needs no refit --
        and ranked among the other N - 1."""
        ref = self.reference(z_threshold)
        if self.cohort is None:
            raise ValueError("a loaded model does not hold its reference: loo needs the model that was fitted")
        host = self._score(self.cohort.values, self.cohort.mask, self.design, True, z_threshold, True) if return_maps else ref["host"]
        return self._result(host, self.cohort.ids, True, z_threshold)

    def deviation(self, cohort_or_vectors, covariates=None, z_threshold: float = 2.0, return_maps: bool = False) -> DeviationResult:
        """Knees that are NOT in the fit -- a ``ThicknessCohort`` on the model's atlas and cartilage, or vectors [M, V] / [V] (arrays or
        device tensors, NaN = missing) -- with their ``covariates`` ([M, c]; [c] for one knee), scored vertex by vertex and ranked among
        the reference's N knees."""
        knees = cohort_or_vectors
        if not isinstance(knees, ThicknessCohort):
            vectors = knees if isinstance(knees, torch.Tensor) else np.asarray(knees, np.float32)
            vectors = vectors.reshape(1, -1) if vectors.ndim == 1 else vectors
            knees = ThicknessCohort(self.atlas, self.kind, chunk=max(len(vectors), 1))
            for row in vectors:
                knees.add_vector(row)
        if knees.kind != self.kind or knees.n_verts != self.n_verts:
            raise ValueError(f"the knees are {knees.kind} maps on {knees.n_verts} vertices, the model is for {self.kind} on {self.n_verts}")
        if len(knees) < 1:
            raise ValueError("there is no knee to score")
        self.reference(z_threshold)                                        # refuses a threshold a loaded model does not hold, before any launch
        host = self._score(knees.values, knees.mask, self.rows(covariates, len(knees)), False, z_threshold, return_maps)
        return self._result(host, knees.ids, False, z_threshold)


# ---- bootstrap intervals ---------------------------------------------------------------------------------------------------------------
BOOTSTRAP_METHODS = ("percentile", "basic", "bca")
MAX_BOOTSTRAP_ROWS = 1 << 20          # rows of one call of the bootstrap kernels: the observed row and the resamples


@dataclass
class BootstrapCounts:
    """``counts``: uint16 [B + 1, N] -- how often knee i enters resample r; row 0 is all ones, the observed data."""
    counts: np.ndarray

    def __len__(self) -> int:
        return int(self.counts.shape[0])


def bootstrap_counts(n_knees: int, n_bootstrap: int, seed: int = 0, blocks=None) -> BootstrapCounts:
    """Resamples for ``bootstrap_ci``: row 0 all ones, every other row the multiplicities of N draws with replacement.  ``blocks``: an int
    label per knee (group, site, ...); knees are then resampled WITHIN a block only, so every row keeps every block's size.  Per block,
    in ascending block label, rows 1.. come from ``np.random.Generator(np.random.PCG64(seed)).integers(0, n_b, size=(B, n_b))``, binned.
    A multiplicity above 65535 is refused."""
    N, B = int(n_knees), int(n_bootstrap)
    if N < 1 or B < 1:
        raise ValueError(f"n_knees and n_bootstrap must be >= 1, got {n_knees}, {n_bootstrap}")
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = np.zeros((B + 1, N), np.int64)
    counts[0] = 1
    for idx in _block_members(blocks, N):
        nb = len(idx)
        draws = rng.integers(0, nb, size=(B, nb))
        counts[1:, idx] = np.bincount((draws + np.arange(B)[:, None] * nb).ravel(), minlength=B * nb).reshape(B, nb)
    if counts.max() > 65535:
        raise ValueError("a knee enters a resample more than 65535 times: the counts are 16-bit")
    return BootstrapCounts(counts.astype(np.uint16))


def _count_rows(counts, make, n_knees: int) -> BootstrapCounts:
    rows = make() if counts is None else counts
    c = np.atleast_2d(rows.counts if isinstance(rows, BootstrapCounts) else np.asarray(rows))
    if c.ndim != 2 or c.shape[1] != n_knees or not np.issubdtype(c.dtype, np.integer) or c.shape[0] < 2:
        raise ValueError(f"counts must be integer rows [B + 1 >= 2, {n_knees}], got {c.dtype} {c.shape}")
    if c.min() < 0 or c.max() > 65535:
        raise ValueError("every count must be 0 .. 65535")
    if not (c[0] == 1).all():
        raise ValueError("row 0 of the counts must be all ones: the observed data")
    return BootstrapCounts(np.ascontiguousarray(c, dtype=np.uint16))


def bootstrap_span(n_rows: int, n_verts: int, budget: int = WORKSPACE_BUDGET) -> int:
    """Vertices per span of ``bootstrap_ci``: what keeps the replicate tile [B + 1][span] within ``budget`` bytes, in whole blocks of 256
    vertices where that leaves one, at least one vertex.  (The quantile step holds a second buffer of the tile's size.)"""
    span = max(int(budget) // (8 * int(n_rows)), 1)
    span = span // 256 * 256 if span >= 256 else span
    return int(min(span, int(n_verts)))


def _bca_probabilities(below, equal, n_finite, acceleration, level: float):
    """(z0 [V], probabilities [2, V]) of the BCa interval, float64 on the host: z0 = Phi^-1((below + (below + equal)) / (2 B')), and with
    z_alpha = Phi^-1((1 - level) / 2) the adjusted probabilities Phi(z0 + (z0 -+ z_alpha) / (1 - a (z0 -+ z_alpha)))."""
    from scipy import special
    alpha = (1.0 - float(level)) / 2.0
    with np.errstate(all="ignore"):
        z0 = special.ndtri((below + (below + equal)).astype(np.float64) / (2.0 * n_finite.astype(np.float64)))
        z_alpha = special.ndtri(alpha)
        z_1alpha = -z_alpha
        num1 = z0 + z_alpha
        p_low = special.ndtr(z0 + num1 / (1.0 - acceleration * num1))
        num2 = z0 + z_1alpha
        p_high = special.ndtr(z0 + num2 / (1.0 - acceleration * num2))
    return z0, np.ascontiguousarray(np.stack([p_low, p_high]))


@dataclass
class BootstrapResult:
    """``estimate`` float64 [V]: the mean ("mean"), the adjusted difference of the larger group label from the smaller ("difference") or the
    slope per unit of ``x`` ("slope"), NaN where the model has no full rank among the knees with a value; ``se`` the standard deviation of
    its finite replicates (n - 1 in the denominator); ``lower``, ``upper`` the ``level`` interval by ``method``; ``n`` the knees with a
    value and ``n_finite`` the finite replicates B' per vertex.  ``z0``, ``acceleration``: the bias correction and the jackknife
    acceleration of "bca", otherwise None.  With ``simultaneous``: ``sup`` the sup-t statistic of every row (entry 0 observed: 0.0),
    ``critical`` its ``level`` quantile over the resamples, and ``lower_simultaneous``, ``upper_simultaneous`` = estimate -+ critical * se,
    a band that covers the whole surface at once; otherwise None."""
    kind: str
    what: str
    estimate: np.ndarray
    se: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    level: float
    method: str
    n: np.ndarray
    n_finite: np.ndarray
    n_bootstrap: int
    z0: Optional[np.ndarray] = None
    acceleration: Optional[np.ndarray] = None
    sup: Optional[np.ndarray] = None
    critical: Optional[float] = None
    lower_simultaneous: Optional[np.ndarray] = None
    upper_simultaneous: Optional[np.ndarray] = None

    IMAGES = ("estimate", "se", "lower", "upper", "n", "n_finite", "z0", "acceleration", "lower_simultaneous", "upper_simultaneous")

    def image(self, atlas, what: str = "estimate"):
        """``atlas.image`` of one of ``IMAGES`` (float32 [H, W], NaN off the surface)."""
        if what not in self.IMAGES:
            raise ValueError(f"no image of {what!r}")
        vec = getattr(self, what)
        if vec is None:
            raise ValueError("the interval is not a bca one" if what in ("z0", "acceleration") else "the interval was computed without simultaneous")
        return atlas.image(np.asarray(vec, np.float32), self.kind)


def _bootstrap_design(x, groups, covariates, intercept: bool, blocks, n_knees: int):
    """(what, design [N, p], the scale the last column was divided by, the int block label of every knee for resampling and strata)."""
    N = n_knees
    if blocks is not None and np.shape(blocks) != (N,):
        raise ValueError(f"blocks must hold one label per knee ({N}), got shape {np.shape(blocks)}")
    labels = np.zeros(N, np.int64) if blocks is None else np.unique(np.asarray(blocks), return_inverse=True)[1].reshape(-1).astype(np.int64)
    if x is not None and groups is not None:
        raise ValueError("give x (a slope) or groups (a difference), not both")
    if x is None and groups is None:
        if covariates is not None or not intercept:
            raise ValueError("the mean map is the intercept alone: covariates and intercept=False need x or groups")
        return "mean", np.ones((N, 1)), 1.0, labels
    if groups is not None:
        g = np.asarray(groups)
        if g.shape != (N,):
            raise ValueError(f"groups must hold one label per knee of the cohort ({N}), got shape {g.shape}")
        levels, which = np.unique(g, return_inverse=True)
        if len(levels) != 2:
            raise ValueError(f"groups must hold exactly two labels, got {len(levels)}")
        _, design, scale = _design_columns(which.reshape(-1).astype(np.float64), covariates, intercept, N)
        return "difference", design, scale, labels * 2 + which.reshape(-1)               # resampled within block and group
    _, design, scale = _design_columns(x, covariates, intercept, N)
    return "slope", design, scale, labels


def bootstrap_ci(cohort: ThicknessCohort, x=None, groups=None, covariates=None, intercept: bool = True, n_bootstrap: int = 2000,
                 level: float = 0.95, method: str = "percentile", simultaneous: bool = False, blocks=None, seed: int = 0, counts=None,
                 batch: Optional[int] = None) -> BootstrapResult:
    """How large is the effect, give or take what?  The nonparametric bootstrap of one coefficient of the per-vertex linear model, over the
    knees with a value at the vertex (include/oai_hip.h, "Bootstrap intervals"; csrc/bootstrap.hip; tests/bootstrap_ref.py).

    With neither ``x`` nor ``groups``: the mean map (the design is the intercept alone) -- on ``LongitudinalCohort.change("rate")`` the loss
    in mm per year with its interval.  With ``groups`` (two labels): the difference of the larger label from the smaller, adjusted for
    ``covariates``; knees are resampled within a group, so no group is ever drawn empty.  With ``x``: the slope per unit of ``x`` as passed.
    ``covariates``, ``intercept`` and the design checks are ``regression_test``'s.  ``blocks``: an int label per knee; knees are resampled
    within a block only.  The resamples are ``bootstrap_counts(N, n_bootstrap, seed, blocks)`` or ``counts`` (a ``BootstrapCounts`` or
    integer rows [B + 1, N], row 0 all ones).

    ``method``: "percentile" (the ``level`` quantiles of the replicates), "basic" (those reflected about the estimate) or "bca" (Efron's
    bias-corrected and accelerated percentiles, the acceleration from a leave-one-knee-out jackknife per resampling stratum).
    ``simultaneous``: also the sup-t band estimate -+ critical * se, which covers all vertices at once.

    The work runs in vertex spans of ``batch`` vertices (default ``bootstrap_span``: the tile [B + 1][span] fits ``WORKSPACE_BUDGET``),
    because a vertex's order statistics need all its replicates at once; the result does not depend on the span.  "percentile" and
    "basic" download once, at the end.  "bca" adds per span one small download (below, equal, B', a) and one upload of [2][span]
    probabilities, since the adjusted probabilities are formed on the host with ``scipy.special``.

    Limits: at most six design columns and one coefficient; percentile-type intervals only (no studentised bootstrap-t); a missing entry
    travels with its knee, so missingness is resampled with the data; the replicates are Monte Carlo, so two seeds give two intervals;
    no significance level or coverage claim is built in."""
    if method not in BOOTSTRAP_METHODS:
        raise ValueError(f"method must be one of {BOOTSTRAP_METHODS}, got {method!r}")
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level!r}")
    N = len(cohort)
    if N < 2:
        raise ValueError("bootstrap_ci needs at least two knees")
    what, design, scale, labels = _bootstrap_design(x, groups, covariates, bool(intercept), blocks, N)
    rows = _count_rows(counts, lambda: bootstrap_counts(N, n_bootstrap, seed, labels), N)
    R = len(rows)
    if R > MAX_BOOTSTRAP_ROWS:
        raise ValueError(f"at most {MAX_BOOTSTRAP_ROWS - 1} resamples are supported, got {R - 1}")
    values, mask = cohort.values, cohort.mask
    V, dev = int(values.shape[1]), values.device
    span = bootstrap_span(R, V) if batch is None else int(batch)
    if span < 1:
        raise ValueError(f"batch must be >= 1 vertices, got {batch!r}")
    span = min(span, V)
    p = design.shape[1]
    design_d, counts_d = torch.from_numpy(np.ascontiguousarray(design)).to(dev), torch.from_numpy(rows.counts).to(dev)
    ws = _lib.workspace("oai_bootstrap_coef", dev, R, span, N, p)
    ws_q = _lib.workspace("oai_column_quantiles", dev, R, span)
    bca = method == "bca"
    if bca:
        strata, n_strata = np.unique(labels, return_inverse=True)[1].reshape(-1).astype(np.int32), len(np.unique(labels))
        strata_d = torch.from_numpy(strata).to(dev)
        jack_d = torch.from_numpy((1 - np.eye(N, dtype=np.int64)).astype(np.uint16)).to(dev)
        ws_j = _lib.workspace("oai_bootstrap_coef", dev, N, span, N, p)
        z0, accel = np.empty(V), np.empty(V)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    estimate, se, quant = f64(V), f64(V), f64(2, V)
    n_valid = torch.empty(V, dtype=torch.int32, device=dev)
    n_finite = torch.empty(V, dtype=torch.int32, device=dev)
    sup = torch.zeros(R, dtype=torch.float64, device=dev) if simultaneous else None
    alpha = (1.0 - level) / 2.0
    for a in range(0, V, span):
        b = min(a + span, V)
        tile = ops.bootstrap_coef(values, design_d, counts_d, 0, R, mask=mask, v0=a, v1=b, workspace=ws, n=n_valid)
        mom = ops.bootstrap_moments(tile)
        estimate[a:b].copy_(tile[0])
        se[a:b].copy_(mom.se)
        n_finite[a:b].copy_(mom.n_finite)
        if simultaneous:
            ops.bootstrap_sup(tile, mom.se, sup)
        if bca:
            jack = ops.bootstrap_coef(values, design_d, jack_d, 0, N, mask=mask, v0=a, v1=b, workspace=ws_j)
            acc = ops.jackknife_acceleration(jack, strata_d, n_strata, mask=mask, v0=a)
            below, equal, finite, accel[a:b] = _download([mom.below, mom.equal, mom.n_finite, acc])
            z0[a:b], probs = _bca_probabilities(below, equal, finite, accel[a:b], level)
            q, _ = ops.column_quantiles(tile, torch.from_numpy(probs).to(dev), first_row=1, workspace=ws_q)
        else:
            q, _ = ops.column_quantiles(tile, (alpha, 1.0 - alpha), first_row=1, workspace=ws_q)
        quant[:, a:b].copy_(q)
    host = _download([estimate, se, quant, n_valid, n_finite] + ([sup] if simultaneous else []))
    est, q = host[0], host[2]
    low, high = (2.0 * est - q[1], 2.0 * est - q[0]) if method == "basic" else (q[0], q[1])
    res = BootstrapResult(kind=cohort.kind, what=what, estimate=est / scale, se=host[1] / scale, lower=low / scale, upper=high / scale, level=level,
                          method=method, n=host[3], n_finite=host[4], n_bootstrap=R - 1)
    if bca:
        res.z0, res.acceleration = z0, accel
    if simultaneous:
        res.sup = host[5]
        res.critical = float(np.quantile(res.sup[1:], level))
        res.lower_simultaneous, res.upper_simultaneous = res.estimate - res.critical * res.se, res.estimate + res.critical * res.se
    return res


# ---- rank tests ------------------------------------------------------------------------------------------------------------------------
# What is and is not classical, for all four tests below:
#   * Where nothing is missing, the t (or F) of the ranks is a monotone function of U (or W, H, rho) under every relabelling, so the
#     permutation p-values are those of the classical exact test.
#   * Where entries are missing, the group sizes at a vertex vary with the labelling; the statistic is then Conover and Iman's t (or F) on
#     ranks (1981), which is still a valid permutation test, and the classical figures are those of the valid knees of the vertex.
#   * Ranks are taken over the whole cohort and never within ``blocks``: blocks restrict the permutations only.  A van Elteren test, which
#     ranks within strata, is not provided.
#   * No asymptotic or exact-table p-value is formed: the permutation p of ``.test`` is the product, and no significance level is built in.
def _rank_scores_method(scores: str, signed: bool = False) -> str:
    if scores not in ("rank", "inormal"):
        raise ValueError(f'scores must be "rank" or "inormal", got {scores!r}')
    return {("rank", False): "rank", ("inormal", False): "inormal", ("rank", True): "signed", ("inormal", True): "signed_inormal"}[(scores, signed)]


def _midranks(x) -> np.ndarray:
    """The midranks of a host vector, float64: scipy.stats.rankdata(method="average") from sorted unique values and their counts."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or not np.isfinite(x).all():
        raise ValueError("a vector to rank must be one finite number per knee")
    _, inverse, counts = np.unique(x, return_inverse=True, return_counts=True)
    last = np.cumsum(counts)                                               # the largest rank of every tie group
    return (last - 0.5 * (counts - 1))[inverse.reshape(-1)]


def _sums_to_host(ranks: "ops.ColumnRanks", labels, n_groups: int):
    """(n_g [G, V], rank sums float64 [G, V] -- a multiple of 1/2, exact --, n_valid [V], tie_term [V]) from ONE ``rank_sums`` call and
    one download."""
    n_g, twice = ops.rank_sums(ranks.twice_rank, labels, n_groups)
    n_g, twice, n_valid, tie_term = _download([n_g, twice, ranks.n_valid, ranks.tie_term])
    return n_g, 0.5 * twice.astype(np.float64), n_valid, tie_term


@dataclass(frozen=True)
class RankSumResult:
    """``test``: the ``PermutationResult`` of ``two_sample_test`` on the ranked cohort, untouched.  Per vertex, over the knees with a value
    there: ``n1``, ``n2`` int32; ``u1`` = R1 - n1 (n1 + 1) / 2, the Mann-Whitney U of group 1 (R1 the sum of its midranks: scipy's
    ``mannwhitneyu(group1, group2).statistic``); ``auc`` = u1 / (n1 n2), the probability of superiority P(a knee of group 1 > one of group 2)
    + P(tie) / 2, NaN where a side is empty; ``tie_term`` int64, the sum over tie groups of t^3 - t."""
    test: PermutationResult
    u1: np.ndarray
    auc: np.ndarray
    n1: np.ndarray
    n2: np.ndarray
    tie_term: np.ndarray


def rank_sum_test(cohort: ThicknessCohort, groups, scores: str = "rank", n_permutations: int = 10000, cluster_threshold: Optional[float] = None,
                  seed: int = 0, blocks=None, permutations=None, batch: Optional[int] = None, tfce=None) -> RankSumResult:
    """The Wilcoxon rank-sum (Mann-Whitney) test per vertex: ``two_sample_test`` of ``cohort.ranked()`` -- robust against the gross outliers
    of an automatic pipeline, which inflate the pooled variance of the plain t -- with the classical U and the probability of superiority
    beside it.  ``scores="inormal"`` runs the test on the rank-based inverse-normal scores instead (``ranked("inormal")``, Blom); ``u1`` and
    ``auc`` are those of the ranks either way.  Every other argument is ``two_sample_test``'s and is passed through.
    Where nothing is missing, the t of the ranks is a monotone function of U under every relabelling, so ``test.p_uncorrected`` is the
    p of the exact Mann-Whitney test (two-sided, over the labellings drawn).  Where entries are missing, n1 and n2 at a vertex vary with
    the labelling, and the statistic is Conover and Iman's t on ranks, still a valid permutation test.  Ranking is over the whole cohort
    and never within ``blocks``; a van Elteren test is not provided.  No asymptotic p-value is formed."""
    g = _as_groups(groups)
    ranked, ranks = cohort._ranked(_rank_scores_method(scores), "blom")
    test = two_sample_test(ranked, g, n_permutations=n_permutations, cluster_threshold=cluster_threshold, seed=seed, blocks=blocks,
                           permutations=permutations, batch=batch, tfce=tfce)
    n_g, R, _, tie_term = _sums_to_host(ranks, np.where(g, 0, 1).astype(np.uint8), 2)
    n1, n2 = n_g[0], n_g[1]
    u1 = R[0] - 0.5 * n1.astype(np.float64) * (n1.astype(np.float64) + 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = np.where((n1 > 0) & (n2 > 0), u1 / (n1.astype(np.float64) * n2.astype(np.float64)), np.nan)
    return RankSumResult(test, u1, auc, n1, n2, tie_term)


@dataclass(frozen=True)
class SignedRankResult:
    """``test``: the ``PermutationResult`` of ``one_sample_test`` on the signed ranks, untouched.  Per vertex: ``w_plus`` and ``w_minus``, the
    sums of the midranks of |value| over the positive and the negative values (scipy's ``wilcoxon(zero_method="wilcox").statistic`` is the
    smaller of the two); ``n_nonzero`` int32, the knees with a value other than zero, which are the ones ranked;
    ``rank_biserial`` = (W+ - W-) / (W+ + W-), NaN where no knee is ranked."""
    test: PermutationResult
    w_plus: np.ndarray
    w_minus: np.ndarray
    n_nonzero: np.ndarray
    rank_biserial: np.ndarray


def signed_rank_test(cohort_a: ThicknessCohort, cohort_b: Optional[ThicknessCohort] = None, scores: str = "rank", n_permutations: int = 10000,
                     cluster_threshold: Optional[float] = None, seed: int = 0, permutations=None, batch: Optional[int] = None,
                     tfce=None) -> SignedRankResult:
    """Wilcoxon's signed-rank test per vertex: ``one_sample_test`` of ``ranked("signed")`` of ``cohort_a`` -- a rate cohort, whose two-visit
    slopes are heavy-tailed -- or, with ``cohort_b``, of ``cohort_a.difference(cohort_b)`` (rows matched by id as ``paired_test`` matches
    them).  A value of exactly zero is dropped before ranking, as scipy's ``zero_method="wilcox"`` does, and is missing in the test.
    ``scores="inormal"``: the test runs on the normal scores of the signed ranks; W+ and W- are those of the ranks either way.  Every
    other argument is ``one_sample_test``'s.  Where nothing is missing (and nothing is zero), the t of the signed ranks is a monotone
    function of W+ under every sign flip, so ``test.p_uncorrected`` is the p of the exact signed-rank test; otherwise the number of ranked
    knees varies from vertex to vertex and not with the flip, and the same holds per vertex.  No asymptotic p-value is formed."""
    base = cohort_a if cohort_b is None else cohort_a.difference(cohort_b)
    ranked, ranks = base._ranked(_rank_scores_method(scores, signed=True), "blom")
    test = one_sample_test(ranked, n_permutations=n_permutations, cluster_threshold=cluster_threshold, seed=seed, permutations=permutations,
                           batch=batch, tfce=tfce)
    _, W, n_valid, _ = _sums_to_host(ranks, None, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        biserial = np.where(n_valid > 0, (W[1] - W[0]) / (W[1] + W[0]), np.nan)
    return SignedRankResult(test, W[1], W[0], n_valid, biserial)


@dataclass(frozen=True)
class KruskalResult:
    """``test``: the ``FResult`` of ``anova_test`` on the ranked cohort, untouched.  ``h`` float64 [V]: the Kruskal-Wallis statistic over the
    knees with a value at the vertex, tie-corrected -- (12 / (n (n + 1)) sum_g R_g^2 / n_g - 3 (n + 1)) / (1 - T / (n^3 - n)), T the tie
    term -- as ``scipy.stats.kruskal`` gives it; NaN where every valid value ties or a level has no knee there.  ``levels``: the sorted
    labels; ``group_n`` int32 [G, V] and ``rank_sum`` float64 [G, V] per level; ``tie_term`` int64 [V]."""
    test: FResult
    h: np.ndarray
    levels: np.ndarray
    group_n: np.ndarray
    rank_sum: np.ndarray
    tie_term: np.ndarray


def kruskal_test(cohort: ThicknessCohort, groups, covariates=None, scores: str = "rank", n_permutations: int = 10000,
                 cluster_threshold: Optional[float] = None, seed: int = 0, blocks=None, permutations=None, batch: Optional[int] = None,
                 tfce=None) -> KruskalResult:
    """The Kruskal-Wallis test per vertex: ``anova_test`` of ``cohort.ranked()`` across the levels of ``groups``, with the classical H beside
    it.  ``covariates`` are passed to ``anova_test`` AS THEY ARE (an analysis of covariance of the ranks); H ignores them.
    ``scores="inormal"``: the F runs on the normal scores; H is that of the ranks either way.  Every other argument is ``anova_test``'s.
    Where nothing is missing and there are no covariates, the F of the ranks is a monotone function of H under every relabelling, so
    ``test.p_uncorrected`` is the p of the exact Kruskal-Wallis test; where entries are missing the level sizes at a vertex vary with the
    labelling and the statistic is Conover and Iman's F on ranks, still a valid permutation test.  Ranking is over the whole cohort and
    never within ``blocks``.  No asymptotic p-value is formed."""
    levels, where = _anova_levels(groups, len(cohort), _n_columns(covariates))
    ranked, ranks = cohort._ranked(_rank_scores_method(scores), "blom")
    test = anova_test(ranked, groups, covariates=covariates, n_permutations=n_permutations, cluster_threshold=cluster_threshold, seed=seed,
                      blocks=blocks, permutations=permutations, batch=batch, tfce=tfce)
    n_g, R, n_valid, tie_term = _sums_to_host(ranks, where.astype(np.uint8), len(levels))
    n, ng = n_valid.astype(np.float64), n_g.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = 12.0 / (n * (n + 1.0)) * (R * R / ng).sum(axis=0) - 3.0 * (n + 1.0)
        h = h / (1.0 - tie_term.astype(np.float64) / (n * n * n - n))
    bad = (n_g == 0).any(axis=0) | (tie_term.astype(np.float64) == n * n * n - n)
    return KruskalResult(test, np.where(bad, np.nan, h), levels, n_g, R, tie_term)


@dataclass(frozen=True)
class SpearmanResult:
    """``test``: the ``RegressionResult`` of ``regression_test`` on the ranked cohort and the ranked regressor, untouched.  ``rho`` float64 [V]
    = ``test.partial_r``: Spearman's rank correlation of thickness and x where no covariates are given and nothing is missing, the partial
    rank correlation given the (ranked) covariates otherwise."""
    test: RegressionResult
    rho: np.ndarray


def spearman_test(cohort: ThicknessCohort, x, covariates=None, scores: str = "rank", n_permutations: int = 10000,
                  cluster_threshold: Optional[float] = None, seed: int = 0, blocks=None, permutations=None, batch: Optional[int] = None,
                  tfce=None) -> SpearmanResult:
    """Spearman's rank correlation per vertex: ``regression_test`` of ``cohort.ranked()`` on the midranks of ``x``, adjusted for the midranks
    of every column of ``covariates`` (a partial rank correlation).  ``scores="inormal"``: thickness enters as normal scores; ``x`` and the
    covariates stay midranks.  Every other argument is ``regression_test``'s.
    ``x`` (and every covariate) is ranked ONCE over all knees and not per vertex: where nothing is missing, ``rho`` is exactly Spearman's
    coefficient, and the t of the ranks is a monotone function of it under every permutation, so ``test.p_uncorrected`` is the p of the
    exact test; where entries are missing, the ranks of x among the valid knees of a vertex are no longer 1 .. n, and ``rho`` is a rank
    regression, not exactly Spearman's coefficient -- still a valid permutation test.  Ranking is over the whole cohort and never within
    ``blocks``.  No asymptotic p-value is formed."""
    rx = _midranks(x)
    cov = None
    if covariates is not None:
        cov = np.asarray(covariates, np.float64)
        cov = _midranks(cov) if cov.ndim == 1 else np.stack([_midranks(cov[:, k]) for k in range(cov.shape[1])], axis=1)
    ranked = cohort.ranked(_rank_scores_method(scores))
    test = regression_test(ranked, rx, covariates=cov, n_permutations=n_permutations, cluster_threshold=cluster_threshold, seed=seed, blocks=blocks,
                           permutations=permutations, batch=batch, tfce=tfce)
    return SpearmanResult(test, test.partial_r)


# ---- cohort PCA ------------------------------------------------------------------------------------------------------------------------
PCA_DROP = 1e-12                      # a component is kept where lambda > 0 and lambda > PCA_DROP * lambda_1: part of the contract
_PCA_ARRAYS = ("mean", "root_weights", "weights", "modes_w", "singular_values", "explained_variance", "explained_variance_ratio")


@dataclass
class PCAScores:
    """One entry per knee scored against a ``ThicknessPCA``: ``scores`` float64 [N', K] (the knee's coordinates on the modes, in
    mm * sqrt(mm^2)); ``t2`` = sum_c score_c^2 / explained_variance_c, Hotelling's T2 INSIDE the model; ``q`` = norm2 - sum_c score_c^2, the
    residual outside it (the squared prediction error of process monitoring), in mm^2 * mm^2, where norm2 is the squared whitened norm of
    the centred knee; ``q_fraction`` = q / norm2; ``n_missing``: the model's vertices at which the knee has no value and was taken to lie
    on the mean.  ``member``: the knees are the model's own (``member_scores``) and their figures optimistic.  No threshold is applied."""
    kind: str
    ids: List[object]
    scores: np.ndarray
    t2: np.ndarray
    q: np.ndarray
    q_fraction: np.ndarray
    n_missing: np.ndarray
    member: bool = False

    def __len__(self) -> int:
        return len(self.ids)


def _pca_record(kind, ids, scores, norm2, explained_variance, n_missing, member) -> PCAScores:
    inside = (scores * scores).sum(axis=1)
    q = norm2 - inside
    with np.errstate(invalid="ignore", divide="ignore"):
        return PCAScores(kind, list(ids), scores, (scores * scores / explained_variance[None, :]).sum(axis=1), q, q / norm2,
                         np.asarray(n_missing, np.int64), member)


class ThicknessPCA:
    """The modes of thickness variation of a cohort and, per knee, two outlier scores: an area-weighted, missing-aware principal
    component analysis of the maps by way of the N x N Gram matrix of the whitened knees (include/oai_hip.h, "Cohort PCA";
    csrc/cohort_pca.hip; tests/cohort_pca_ref.py).  ``fit`` keeps ``mean`` [V] (mm), ``modes_mm`` [K, V] (orthonormal under the weighted
    inner product sum_v w_v x_v y_v; NaN at excluded vertices), ``singular_values`` [K], ``explained_variance`` = lambda / (N - 1),
    ``explained_variance_ratio`` = lambda / trace G, ``scores`` [N, K], ``ids``, ``n_excluded``, ``weights`` [V], and the settings of a
    derived cohort (``smoothing``, ``ranking``, ``change``): ``cohort.ranked("inormal").pca()`` is the correlation-type analysis.

    Limits.  A missing entry contributes 0 after centring -- mean imputation -- and is counted in ``n_missing`` (per knee) and
    ``n_excluded`` (vertices with fewer than ``min_valid`` knees).  ``member_scores`` is not leave-one-out.  K is the caller's choice: no
    parallel analysis.  The eigendecomposition runs on the host.  Equal eigenvalues leave their modes defined only up to rotation.  No
    fp64 MFMA path.  No thresholds."""

    def __init__(self, surface: ThicknessCohort, mean, root_weights, weights, modes_w, singular_values, explained_variance,
                 explained_variance_ratio, n_knees: int, n_excluded: int, min_valid: int):
        self.surface = surface
        self.atlas, self.kind, self.device, self.n_verts = surface.atlas, surface.kind, surface.device, surface.n_verts
        self.mean, self.root_weights, self.weights = (np.asarray(a, np.float64) for a in (mean, root_weights, weights))
        self.modes_w = np.ascontiguousarray(modes_w, np.float64)           # the root-weighted modes R [K, V], orthonormal rows
        self.singular_values, self.explained_variance, self.explained_variance_ratio = (
            np.asarray(a, np.float64) for a in (singular_values, explained_variance, explained_variance_ratio))
        self.n_knees, self.n_excluded, self.min_valid = int(n_knees), int(n_excluded), int(min_valid)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.modes_mm = np.where(self.root_weights[None, :] != 0.0, self.modes_w / self.root_weights[None, :], np.nan)
        self.smoothing, self.ranking, self.change = surface.smoothing, surface.ranking, surface.change
        self.ids: List[object] = []
        self.scores: Optional[np.ndarray] = None          # [N, K] of the members; None on a model that was loaded
        self.gram_diagonal: Optional[np.ndarray] = None
        self.member_missing: Optional[np.ndarray] = None
        self.eigh_seconds = 0.0                           # the host eigendecomposition of the last fit
        self._device: dict = {}

    @property
    def n_components(self) -> int:
        return int(self.modes_w.shape[0])

    def _dev(self, name: str) -> torch.Tensor:
        if name not in self._device:
            self._device[name] = torch.from_numpy(np.ascontiguousarray(getattr(self, name))).to(self.device)
        return self._device[name]

    @classmethod
    def fit(cls, cohort: ThicknessCohort, n_components: int = 10, weights="area", min_valid: int = 2) -> "ThicknessPCA":
        """The model of ``cohort``.  ``weights``: "area" (``cohort.vertex_areas()``, mm^2), "uniform" (ones) or an array [V] of finite
        values >= 0.  A vertex at which fewer than ``min_valid`` (>= 1) knees have a value gets weight 0 and is counted in ``n_excluded``.
        Components are kept where lambda_c > 0 and lambda_c > 1e-12 lambda_1, and K = min(n_components, kept).  On the device: the mean
        (``ops.group_prepare``), the whitening, the Gram matrix and the modes; on the host, after ONE download of the [N, N] Gram matrix
        (with the per-vertex counts behind it), ``np.linalg.eigh``; the modes come back in a second, final download."""
        import time
        N, V, dev = len(cohort), cohort.n_verts, cohort.device
        if N < 2:
            raise ValueError("a PCA needs at least two knees")
        if int(n_components) < 1 or int(min_valid) < 1:
            raise ValueError(f"n_components and min_valid must be >= 1, got {n_components!r}, {min_valid!r}")
        if isinstance(weights, str):
            if weights not in ("area", "uniform"):
                raise ValueError(f"weights must be 'area', 'uniform' or an array [{V}], got {weights!r}")
            w = np.asarray(cohort.vertex_areas(), np.float64) if weights == "area" else np.ones(V)
        else:
            w = np.asarray(weights, np.float64)
        if w.shape != (V,) or not np.isfinite(w).all() or (w < 0.0).any():
            raise ValueError(f"weights must be {V} finite values >= 0")
        prep = ops.group_prepare(cohort.values, cohort.mask)
        out = prep.n < int(min_valid)                                      # a select on the device: the counts are not brought to the host first
        rw_d = torch.where(out, torch.zeros((), dtype=torch.float64, device=dev), torch.from_numpy(np.sqrt(w)).to(dev))
        A = ops.cohort_whiten(cohort.values, cohort.mask, prep.mean, rw_d)
        missing = ((cohort.mask == 0) & (rw_d != 0.0)[None, :]).sum(dim=1)
        G, mean, rw, missing, n_excluded = _download([ops.rows_cross(A, workspace=ops.rows_cross_workspace(N, N, V, dev)), prep.mean, rw_d, missing,
                                                      out.sum().reshape(1)])
        t0 = time.perf_counter()
        lam, U = np.linalg.eigh(G)
        seconds = time.perf_counter() - t0
        lam, U = lam[::-1], U[:, ::-1]
        kept = int(((lam > 0.0) & (lam > PCA_DROP * lam[0])).sum())
        K = min(int(n_components), kept)
        if K < 1:
            raise ValueError("the cohort has no variance: every whitened knee is zero")
        lam, U = lam[:K].copy(), np.ascontiguousarray(U[:, :K])
        s = np.sqrt(lam)
        R = ops.rows_combine(torch.from_numpy(np.ascontiguousarray(U.T / s[:, None])).to(dev), A).cpu().numpy()
        for c in range(K):                                                  # the sign rule; the lowest vertex wins ties (np.argmax)
            if R[c, int(np.argmax(np.abs(R[c])))] < 0.0:
                R[c], U[:, c] = -R[c], -U[:, c]
        model = cls(cohort, mean, rw, w, R, s, lam / (N - 1), lam / G.diagonal().sum(), N, int(n_excluded[0]), int(min_valid))
        model.ids, model.scores, model.gram_diagonal, model.member_missing = list(cohort.ids), s[None, :] * U, G.diagonal().copy(), missing
        model.eigh_seconds = seconds
        return model

    # -- scoring ----------------------------------------------------------------------------------------------------------------------------
    def transform(self, cohort_or_vectors) -> PCAScores:
        """Knees scored against the model -- a ``ThicknessCohort`` on the model's atlas and cartilage, or vectors [M, V] / [V] (arrays or
        device tensors, NaN = missing): each is whitened with the model's mean and root weights, its scores are its ordered dots with the
        root-weighted modes, and Q is read from its squared norm.  Two small launches and ONE download."""
        knees = cohort_or_vectors
        if not isinstance(knees, ThicknessCohort):
            vectors = knees if isinstance(knees, torch.Tensor) else np.asarray(knees, np.float32)
            vectors = vectors.reshape(1, -1) if vectors.ndim == 1 else vectors
            knees = ThicknessCohort(self.atlas, self.kind, chunk=max(len(vectors), 1))
            for row in vectors:
                knees.add_vector(row)
        if knees.kind != self.kind or knees.n_verts != self.n_verts:
            raise ValueError(f"the knees are {knees.kind} maps on {knees.n_verts} vertices, the model is for {self.kind} on {self.n_verts}")
        if len(knees) < 1:
            raise ValueError("there is no knee to score")
        rw_d = self._dev("root_weights")
        A, norm2 = ops.cohort_whiten(knees.values, knees.mask, self._dev("mean"), rw_d, return_norm2=True)
        # the split form: one knee against K modes is a single tile, which one workgroup would otherwise walk chunk by chunk
        scores = ops.rows_cross(A, self._dev("modes_w"), workspace=ops.rows_cross_workspace(len(knees), self.n_components, self.n_verts, self.device))
        missing = ((knees.mask == 0) & (rw_d != 0.0)[None, :]).sum(dim=1)
        scores, norm2, missing = _download([scores, norm2, missing])
        return _pca_record(self.kind, knees.ids, scores, norm2, self.explained_variance, missing, False)

    def member_scores(self) -> PCAScores:
        """The record of ``transform`` for the model's own knees, from the Gram matrix' diagonal and ``scores``, with no launch.  OPTIMISTIC:
        every knee helped to shape the modes it is scored on; there is no leave-one-out."""
        if self.scores is None:
            raise ValueError("a loaded model does not hold its members: member_scores needs the model that was fitted")
        return _pca_record(self.kind, self.ids, self.scores, self.gram_diagonal, self.explained_variance, self.member_missing, True)

    def reconstruct(self, scores) -> np.ndarray:
        """float64 [N', V]: the maps in mm that ``scores`` [N', K] (or [K]) stand for, mean + sum_c score_c modes_mm_c by way of
        ``ops.rows_combine``; NaN at excluded vertices."""
        sc = np.asarray(scores, np.float64)
        sc = np.ascontiguousarray(sc.reshape(1, -1) if sc.ndim == 1 else sc)
        if sc.ndim != 2 or sc.shape[1] != self.n_components or sc.shape[0] < 1:
            raise ValueError(f"scores must be [N', {self.n_components}], got {sc.shape}")
        part = ops.rows_combine(torch.from_numpy(sc).to(self.device), self._dev("modes_w")).cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.root_weights[None, :] != 0.0, self.mean[None, :] + part / self.root_weights[None, :], np.nan)

    def image(self, atlas, mode: int = 0):
        """``atlas.image`` of physical mode ``mode`` (float32 [H, W], NaN off the surface and at excluded vertices)."""
        if not 0 <= int(mode) < self.n_components:
            raise ValueError(f"no mode {mode!r}: the model has {self.n_components}")
        return atlas.image(np.asarray(self.modes_mm[int(mode)], np.float32), self.kind)

    # -- persistence --------------------------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """Write the model as one ``.npz`` -- everything ``transform`` and ``reconstruct`` need -- without the thickness maps and the
        members' scores."""
        state = {name: getattr(self, name) for name in _PCA_ARRAYS}
        state.update(kind=np.asarray(self.kind), n_knees=np.asarray(self.n_knees, np.int64), n_excluded=np.asarray(self.n_excluded, np.int64),
                     min_valid=np.asarray(self.min_valid, np.int64))
        NormativeModel.write_state(path, state)

    @classmethod
    def load(cls, path, atlas) -> "ThicknessPCA":
        """The model that ``save`` wrote, on ``atlas`` (whose inner mesh of the model's cartilage must have the model's vertices).  It scores
        new knees; ``member_scores`` needs the members and is not available."""
        s = NormativeModel.read_state(path)
        kind = str(s["kind"])
        surface = ThicknessCohort(atlas, kind)
        if int(s["mean"].shape[0]) != surface.n_verts:
            raise ValueError(f"the model has {int(s['mean'].shape[0])} vertices, the atlas' {kind} inner mesh {surface.n_verts}")
        return cls(surface, *(s[name] for name in _PCA_ARRAYS), int(s["n_knees"]), int(s["n_excluded"]), int(s["min_valid"]))

