"""GPU: the cohort-PCA kernels (csrc/cohort_pca.hip) against their numpy restatement (tests/cohort_pca_ref.py) TO THE BIT -- whitening,
squared norms, the ordered dot in both execution forms, the ordered combine -- at the shapes where the order can go wrong, and
stats.ThicknessPCA end to end on a small icosphere cohort: the fit equals the restatement's to the bit (both run np.linalg.eigh on the
same host from a bit-identical Gram matrix), planted modes are found, a painted knee stands out in Q and not in T2.

Tolerances.  Everything a kernel writes is held to the bit.  What the host derives twice by different routes (transform of the members
against their fitted scores; Q against an explicit residual; a full-rank reconstruction against the data) is held to GATE = 1e-10 of the
largest magnitude involved, the house gate; each test prints what it measured.
Measured on an MI355X: transform of the members against the fitted scores 2.1e-15 of the largest, q against member_scores 1.0e-15, q
against the explicit residual 1.1e-15, reconstruct against numpy 8.9e-16 mm, a full-rank reconstruction against the data 4.2e-15 mm;
the planted modes are found with |dot| 0.996 and 0.988 (the bound the study sets is 0.9); the painted knee gains 1.013 of its paint's
energy in q (the bound is within 10 %, reasoned in that test).

Not checked here: that nothing synchronises inside ``fit`` beyond its two downloads.  The neighbouring tests (normative, bootstrap, rank)
have no harness for "one download", so there is nothing to follow."""
import functools

import numpy as np
import pytest
import torch

import cohort_pca_ref as pref
from cohort_cases import cohort as _cohort, dev, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

T = 64                                            # csrc/cohort_pca.hip, kTile: edge of a workgroup's tile of rows_cross
OWN = 4                                           # kOwn: rows and columns per thread
VERTS = (1, 511, 512, 513, 1025, 1537)            # both sides of a chunk (512); several chunks with a short last one
KNEES = (2, 3, T - 1, T, T + 1, 2 * T + 2)
GATE = 1e-10


@functools.lru_cache(maxsize=None)
def _case(N, V, masked):
    """(Y, mask, mean, rw) and the restated A, norm2, G: values over several decades so that the order of the sums shows, one vertex
    without a valid knee (its mean is NaN), one root weight of zero, a NaN under a set mask bit."""
    rng = np.random.default_rng([N, V, int(masked), 11])
    Y = (rng.normal(2.0, 0.6, size=(N, V)) * 10.0 ** rng.integers(-2, 3, size=(1, V))).astype(np.float32)
    mask = (rng.random((N, V)) >= 0.1) if masked else None
    rw = np.sqrt(rng.uniform(0.2, 1.8, size=V))
    if V >= 8:
        if masked:
            mask[:, 3] = False
            mask[N // 2, 6] = True
        else:
            Y[:, 3] = np.nan
        Y[N // 2, 6] = np.nan
        rw[5] = 0.0
    mean, _ = pref.counted_mean(Y, mask)
    A = pref.whiten(Y, mask, mean, rw)
    out = (Y, mask, mean, rw, A, pref.norm2(A), pref.ordered_dot(A, A))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _whiten(Y, mask, mean, rw, norm2=True):
    from oai_analysis_2_amd import ops
    return ops.cohort_whiten(dev(Y), None if mask is None else dev(mask), dev(mean), dev(rw), return_norm2=norm2)


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("V", VERTS)
@pytest.mark.parametrize("N", KNEES)
def test_whiten_cross_and_combine_equal_the_restatement_to_the_bit(N, V, masked):
    from oai_analysis_2_amd import ops
    Y, mask, mean, rw, A, norm2, G = _case(N, V, masked)
    if V >= 8:
        assert np.isnan(mean[3]) and (A[:, [3, 5]] == 0.0).all() and A[N // 2, 6] == 0.0 and np.isfinite(A).all()
    a_d, n2_d = _whiten(Y, mask, mean, rw)
    same_bits(a_d, A, "whitened")
    same_bits(n2_d, norm2, "norm2")
    same_bits(_whiten(Y, mask, mean, rw, norm2=False), A, "whitened, no norm2")
    walk = ops.rows_cross(a_d)
    ws = ops.rows_cross_workspace(N, N, V, a_d.device)
    assert ws is not None and ws.numel() == ((N + T - 1) // T) ** 2 * ((V + 511) // 512) * T * T * 8
    split = ops.rows_cross(a_d, workspace=ws)
    same_bits(walk, G, "Gram matrix, walk form")
    same_bits(split, G, "Gram matrix, split form")
    assert torch.equal(walk, walk.T) and np.array_equal(G.diagonal(), norm2)
    K = min(5, N)
    coef = np.random.default_rng([N, V]).normal(size=(K, N))
    same_bits(ops.rows_combine(dev(coef), a_d), pref.combine(coef, A), "combine")


@pytest.mark.parametrize("n_a,n_b,V", ((T + 6, 2 * T + 2, 1025), (2 * T + 1, 3, 513), (1, T + 1, 1537), (5, 1, 1)))
def test_rectangular_cross_in_both_forms(n_a, n_b, V):
    from oai_analysis_2_amd import ops
    rng = np.random.default_rng([n_a, n_b, V])
    a = rng.normal(size=(n_a, V)) * 10.0 ** rng.integers(-3, 4, size=(n_a, V))
    b = rng.normal(size=(n_b, V)) * 10.0 ** rng.integers(-3, 4, size=(n_b, V))
    want = pref.ordered_dot(a, b)
    a_d, b_d = dev(a), dev(b)
    same_bits(ops.rows_cross(a_d, b_d), want, "walk")
    same_bits(ops.rows_cross(a_d, b_d, workspace=ops.rows_cross_workspace(n_a, n_b, V, a_d.device)), want, "split")
    same_bits(ops.rows_cross(b_d, a_d), np.ascontiguousarray(want.T), "swapped")


def test_walk_and_split_agree_run_to_run_and_the_mirror_is_a_computed_triangle():
    from oai_analysis_2_amd import ops
    N, V = 2 * T + 2, 1537
    a_d = dev(_case(N, V, True)[4])
    ws = ops.rows_cross_workspace(N, N, V, a_d.device)
    walk = [ops.rows_cross(a_d) for _ in range(2)]
    split = [ops.rows_cross(a_d, workspace=ws) for _ in range(2)]
    assert torch.equal(walk[0], walk[1]) and torch.equal(split[0], split[1]) and torch.equal(walk[0], split[0])
    full = ops.rows_cross(a_d, a_d.clone())                              # not symmetric to the entry point: every tile is computed
    assert torch.equal(walk[0], full) and torch.equal(ops.rows_cross(a_d, a_d.clone(), workspace=ws), full)
    assert torch.equal(ops.rows_cross(a_d, a_d), full)                   # b given as the same tensor: mirrored as well
    with pytest.raises(Exception, match="workspace"):
        ops.rows_cross(a_d, workspace=ws[:ws.numel() - 1])
    big = ops.rows_cross_workspace(17 * T, 16 * T, 8, a_d.device)
    assert big is None                                                    # more than 256 tiles: that shape walks with or without one


def test_python_layer_refuses_what_its_neighbours_refuse():
    from oai_analysis_2_amd import ops
    a = torch.zeros((4, 10), dtype=torch.float64, device="cuda")
    y = torch.zeros((4, 10), dtype=torch.float32, device="cuda")
    v = torch.zeros(10, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception, match="float64"):
        ops.rows_cross(a.float())
    with pytest.raises(Exception, match="GPU"):
        ops.rows_cross(a.cpu())
    with pytest.raises(ValueError, match="same vertices"):
        ops.rows_cross(a, a[:, :5])
    with pytest.raises(ValueError, match="needs 10 rows"):
        ops.rows_combine(a, a)
    with pytest.raises(ValueError, match="mean must be"):
        ops.cohort_whiten(y, None, v[:5], v)
    with pytest.raises(Exception, match="root_weights must be torch.float64"):
        ops.cohort_whiten(y, None, v, v.float())
    with pytest.raises(ValueError, match="mask must have"):
        ops.cohort_whiten(y, torch.ones((4, 9), dtype=torch.uint8, device="cuda"), v, v)
    assert ops.rows_cross(a[:, ::2]).shape == (4, 4)                      # a view is made contiguous, as everywhere


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
N_KNEES = 32


@functools.lru_cache(maxsize=None)
def _study():
    """32 knees on the 642-vertex icosphere (two chunks: 512 + 130): two planted modes, x and y of the vertex (orthogonal under the area
    inner product up to the mesh's asymmetry) with amplitudes 1.0 and 0.5 mm, noise of 0.05 mm, 10 % missing; the fitted cohort, the
    model with four components and the restatement's fit."""
    atlas = sphere_atlas()
    verts = np.asarray(atlas.inner["FC"].verts, np.float64) / 20.0
    rng = np.random.default_rng(2024)
    planted = np.stack([verts[:, 0], verts[:, 1]])
    amp = rng.normal(size=(N_KNEES, 2)) * np.array([1.0, 0.5])
    Y = (2.5 + amp @ planted + 0.05 * rng.normal(size=(N_KNEES, verts.shape[0]))).astype(np.float32)
    mask = rng.random(Y.shape) >= 0.10
    cohort = _cohort(atlas, Y, mask=mask, chunk=7)
    areas = np.asarray(cohort.vertex_areas(), np.float64)
    for a in (Y, mask, planted, areas):
        a.setflags(write=False)
    return atlas, cohort, Y, mask, planted, areas, cohort.pca(4), pref.fit(Y, mask, areas, n_components=4)


def test_fit_equals_the_restatement_to_the_bit_and_finds_the_planted_modes():
    from oai_analysis_2_amd import stats
    atlas, cohort, Y, mask, planted, areas, pca, want = _study()
    assert isinstance(pca, stats.ThicknessPCA) and pca.n_components == 4 and pca.ids == cohort.ids and pca.n_excluded == want.n_excluded == 0
    for name in ("mean", "singular_values", "explained_variance", "explained_variance_ratio", "scores", "modes_mm"):
        same_bits(getattr(pca, name), getattr(want, name), name)
    same_bits(pca.modes_w, want.modes_w, "root-weighted modes")
    same_bits(pca.root_weights, want.rw, "root weights")
    same_bits(pca.weights, areas, "weights")
    same_bits(pca.gram_diagonal, want.G.diagonal().copy(), "diagonal of G")
    for c in range(2):                                                     # modes_mm is orthonormal under the area inner product
        dot = abs((pca.modes_mm[c] * areas * planted[c]).sum()) / np.sqrt((areas * planted[c] ** 2).sum())
        print(f"mode {c}: |dot| with the planted mode under the area inner product {dot:.4f}")
        assert dot >= 0.9
    gram = (pca.modes_mm * areas[None, :]) @ pca.modes_mm.T
    assert np.abs(gram - np.eye(4)).max() <= GATE
    assert pca.explained_variance_ratio[:2].sum() > 0.9 and pca.smoothing is None and pca.ranking is None
    uniform = cohort.pca(2, weights="uniform")
    same_bits(uniform.scores, pref.fit(Y, mask, np.ones(Y.shape[1]), n_components=2).scores, "uniform weights")
    ranked = cohort.ranked("inormal")
    assert ranked.pca(2).ranking is ranked.ranking                        # the settings of a derived cohort travel with the model


def test_min_valid_excludes_vertices_on_the_device():
    atlas, cohort, Y, mask, planted, areas, _, _ = _study()
    mask = mask.copy()
    mask[:, 9] = False
    mask[:, 21] = np.arange(N_KNEES) == 4
    mask[:, 500:520] &= (np.arange(N_KNEES) < 3)[:, None]
    got, want = _cohort(atlas, Y, mask=mask, chunk=7).pca(3, min_valid=4), pref.fit(Y, mask, areas, n_components=3, min_valid=4)
    assert got.n_excluded == want.n_excluded == 22 and np.isnan(got.mean[9]) and np.isnan(got.modes_mm[:, 9]).all()
    for name in ("mean", "singular_values", "scores", "modes_mm", "explained_variance_ratio"):
        same_bits(getattr(got, name), getattr(want, name), name)
    assert np.isfinite(got.scores).all() and np.isfinite(got.singular_values).all()


def test_transform_member_scores_and_reconstruct():
    atlas, cohort, Y, mask, planted, areas, pca, want = _study()
    rec, ref = pca.transform(cohort), pref.transform(want, Y, mask)
    for name in ("scores", "t2", "q", "q_fraction"):
        same_bits(getattr(rec, name), getattr(ref, name), "transform " + name)
    assert np.array_equal(rec.n_missing, ref.n_missing) and np.array_equal(rec.n_missing, (~mask).sum(axis=1)) and rec.ids == cohort.ids
    largest = np.abs(pca.scores).max()
    e_scores = np.abs(rec.scores - pca.scores).max() / largest
    members = pca.member_scores()
    e_q = np.abs(rec.q - members.q).max() / pca.gram_diagonal.max()
    print(f"transform of the members against the fitted scores: {e_scores:.2e} of the largest; q against member_scores: {e_q:.2e}")
    assert e_scores <= GATE and e_q <= GATE and members.member and not rec.member
    assert np.array_equal(members.scores, pca.scores) and np.array_equal(members.n_missing, rec.n_missing)
    assert np.abs(members.t2.sum() - (N_KNEES - 1) * 4) <= GATE * N_KNEES * 4
    # one knee as a bare vector (NaN = missing) is the same record
    row = np.where(mask[7], Y[7], np.nan).astype(np.float32)
    one = pca.transform(row)
    assert len(one) == 1 and np.array_equal(one.scores[0], rec.scores[7]) and one.q[0] == rec.q[7] and one.n_missing[0] == rec.n_missing[7]
    # Q is the squared norm of the explicit residual, and reconstruct is mean + scores . modes
    resid = want.A - rec.scores @ pca.modes_w
    e_resid = np.abs(rec.q - (resid * resid).sum(axis=1)).max() / pca.gram_diagonal.max()
    back = pca.reconstruct(rec.scores)
    e_back = np.abs(back - (pca.mean[None, :] + rec.scores @ pca.modes_mm)).max()
    centred = (back - pca.mean[None, :]) + resid / pca.root_weights[None, :]
    e_centred = np.abs(np.where(mask, centred - (Y.astype(np.float64) - pca.mean[None, :]), 0.0)).max()
    print(f"q against the explicit residual {e_resid:.2e}; reconstruct against numpy {e_back:.2e} mm; reconstruction plus residual against "
          f"the centred data on valid entries {e_centred:.2e} mm")
    assert e_resid <= GATE and e_back <= GATE and e_centred <= GATE and pca.reconstruct(rec.scores[3]).shape == (1, Y.shape[1])
    # with every component kept the model spans the (mean-imputed) members: the reconstruction IS the data where it is valid
    full = cohort.pca(N_KNEES)
    assert full.n_components == N_KNEES - 1
    e_full = np.abs(np.where(mask, full.reconstruct(full.scores) - Y.astype(np.float64), 0.0)).max()
    print(f"full-rank reconstruction against the data on valid entries {e_full:.2e} mm; the members' largest q_fraction "
          f"{full.member_scores().q_fraction.max():.2e}")
    assert e_full <= GATE * 4.0                                            # values up to 4 mm
    with pytest.raises(ValueError, match="scores must be"):
        pca.reconstruct(np.zeros((2, 3)))


def test_a_painted_knee_stands_out_in_q_and_not_in_t2():
    """A knee that is NOT in the fit: the member of median T2 with 1.5 mm painted on the cap z > 0.8 (61 vertices, about a tenth of the
    surface).  Two components, so that the model is the planted plane and nothing of the noise.  The cap is symmetric about z, so its
    dots with the planted modes x and y vanish up to the mesh's asymmetry and the 10 % of holes: the paint lies outside the model, T2
    does not see it and Q gains the paint's own energy E = sum over the valid cap of 1.5^2 area_v.  The gain q - q_clean = E + 2 r.p - (the
    part of p inside the model), r the clean knee's residual: r.p is noise (0.05 mm) against 1.5 mm over the cap, under 1 % of E, and
    the part inside the model is a few per cent of E at most: the gain is held to E within 10 %.  The other knees' q is not small --
    mean imputation leaves the tenth of a knee's own in-model signal that its holes took outside the model -- so the test asks for the
    largest q and for this gain, not for a ratio to the others."""
    atlas, cohort, Y, mask, planted, areas, _, _ = _study()
    pca = cohort.pca(2)
    base = int(np.argsort(pca.member_scores().t2)[N_KNEES // 2])
    verts = np.asarray(atlas.inner["FC"].verts, np.float64) / 20.0
    cap = verts[:, 2] > 0.8
    painted = np.where(mask[base], Y[base] + np.where(cap, 1.5, 0.0), np.nan).astype(np.float32)
    rows = np.concatenate([np.where(mask, Y, np.nan).astype(np.float32), painted[None, :]])
    rec = pca.transform(rows)
    energy = (1.5 ** 2 * areas * (cap & mask[base])).sum()
    gain = rec.q[-1] - rec.q[base]
    print(f"painted knee: q {rec.q[-1]:.4g} (its clean self {rec.q[base]:.4g}, others at most {rec.q[:-1].max():.4g}), gain / paint energy "
          f"{gain / energy:.4f}, q_fraction {rec.q_fraction[-1]:.3f}, t2 {rec.t2[-1]:.3g} (its clean self {rec.t2[base]:.3g}, others at most "
          f"{rec.t2[:-1].max():.3g})")
    assert int(np.argmax(rec.q)) == N_KNEES and abs(gain - energy) <= 0.1 * energy
    assert rec.t2[-1] < rec.t2[:-1].max() and rec.q_fraction[-1] > rec.q_fraction[:-1].max()


class _Knee(dict):
    """What ThicknessCohort.add reads of a KneeThickness."""
    errors = {}
    coverage = {}


def test_pca_stream_yields_the_records_of_transform():
    from oai_analysis_2_amd import dask_processing
    atlas, cohort, Y, mask, planted, areas, pca, _ = _study()
    rec = pca.transform(cohort)
    knees = [(100 + i, _Knee(FC=np.where(mask[i], Y[i], np.nan).astype(np.float32))) for i in (0, 5, 31)]
    failed = _Knee(FC=Y[0])
    failed.errors = {"FC": "no mesh"}
    got = list(dask_processing.pca_stream(iter(knees + [(7, failed)]), {"FC": pca}))
    assert [index for index, _ in got] == [100, 105, 131, 7]
    for (index, found), i in zip(got[:3], (0, 5, 31)):
        one = found["FC"]
        assert one.ids == [index] and one.n_missing[0] == rec.n_missing[i]
        for name in ("scores", "t2", "q", "q_fraction"):
            assert np.array_equal(getattr(one, name)[0], getattr(rec, name)[i]), name
    lost = got[3][1]["FC"]
    assert lost.n_missing[0] == Y.shape[1] and lost.q[0] == 0.0 and (lost.scores == 0.0).all()
