"""CPU: the brute-force restatement of threshold-free cluster enhancement (tests/graph_tfce_ref.py) held to something other than itself --
sums written out by hand, the integral the sum approximates, extents worked out by hand, and the two symmetries of the definition."""
import numpy as np
import pytest

import graph_tfce_ref as tref
from cohort_cases import same_bits


def _plateau(L, T, pad=7):
    row = np.zeros(L + 2 * pad)
    row[pad:pad + L] = T
    return row, slice(pad, pad + L)


def test_a_plateau_gives_the_sum_written_out_by_hand():
    L, dh = 61, 0.25
    row, inside = _plateau(L, 1.0)
    off, nbr = tref.path_graph(len(row))
    got, clipped = tref.tfce(row[None], off, nbr, dh=dh, E=1.0, H=2.0)
    want = 0.0
    for h in (1.0, 0.75, 0.5, 0.25):                                       # descending, one accumulator
        want = want + ((float(L) * (h * h)) * dh)
    assert want == 28.59375
    assert (got[0, inside] == want).all() and clipped[0] == 0
    outside = np.ones(len(row), bool)
    outside[inside] = False
    same_bits(got[0, outside], np.zeros(outside.sum()), "outside the plateau")       # +0.0, not -0.0


@pytest.mark.parametrize("E", [0.5, 1.0])
@pytest.mark.parametrize("H", [1.0, 2.0])
def test_a_plateau_stays_within_the_bound_of_a_right_endpoint_sum(E, H):
    """The integrand L^E h^H rises with h, so the right-endpoint sum S over (0, T] exceeds the integral L^E T^(H+1) / (H+1) by at most
    its last term's height times the step, L^E T^H dh, when T is a multiple of dh; the error falls as dh does."""
    L, T = 61, 2.0
    row, inside = _plateau(L, T)
    off, nbr = tref.path_graph(len(row))
    integral = L ** E * T ** (H + 1) / (H + 1)
    excess = []
    for dh in (0.25, 0.125, 0.0625):
        got, _ = tref.tfce(row[None], off, nbr, dh=dh, E=E, H=H)
        S = got[0, inside]
        assert (S == S[0]).all()
        excess.append(S[0] - integral)
        assert 0.0 <= excess[-1] <= L ** E * T ** H * dh, (dh, excess[-1])
    assert excess[0] > excess[1] > excess[2] > 0.0


def test_two_hills_and_a_saddle_see_the_extents_worked_out_by_hand():
    """0 | hill A: three vertices at 1.0 | saddle: two at 0.5 | hill B: four at 1.5 | 0, dh = 0.25, E = H = 1, vertex counts.
    A vertex of A: extent 3 at 1.0 and 0.75 (B is there but apart), 9 at 0.5 and 0.25 (the saddle joins everything).
    A vertex of B: 4 from 1.5 down to 0.75, then 9.  The saddle: 9 at 0.5 and 0.25."""
    row = np.array([0, 1.0, 1.0, 1.0, 0.5, 0.5, 1.5, 1.5, 1.5, 1.5, 0, 0])
    off, nbr = tref.path_graph(len(row))
    got, _ = tref.tfce(row[None], off, nbr, dh=0.25, E=1.0, H=1.0)

    def by_hand(extents):                                                  # [(level, extent)] in descending level
        acc = 0.0
        for h, e in extents:
            acc = acc + ((float(e) * h) * 0.25)
        return acc
    a = by_hand([(1.0, 3), (0.75, 3), (0.5, 9), (0.25, 9)])
    b = by_hand([(1.5, 4), (1.25, 4), (1.0, 4), (0.75, 4), (0.5, 9), (0.25, 9)])
    s = by_hand([(0.5, 9), (0.25, 9)])
    assert got[0].tolist() == [0.0, a, a, a, s, s, b, b, b, b, 0.0, 0.0]
    # the same with weights: A weighs 2 per vertex, the rest 1, in units of a half
    w = np.ones(len(row), np.int64)
    w[1:4] = 2
    got, _ = tref.tfce(row[None], off, nbr, dh=0.25, E=1.0, H=1.0, weights=w, unit=0.5)
    assert got[0, 2] == by_hand([(1.0, 3.0), (0.75, 3.0), (0.5, 6.0), (0.25, 6.0)])


def _random_graph(V, rng):
    """A ring with random chords, as symmetric CSR with ascending neighbour lists."""
    pairs = {(i, (i + 1) % V) for i in range(V)} | {tuple(rng.integers(0, V, 2)) for _ in range(V)}
    nb = [set() for _ in range(V)]
    for a, b in pairs:
        if a != b:
            nb[a].add(int(b))
            nb[b].add(int(a))
    off = np.concatenate([[0], np.cumsum([len(s) for s in nb])]).astype(np.int32)
    return off, np.concatenate([sorted(s) for s in nb]).astype(np.int32)


def _noise(V, rng):
    tile = rng.normal(0.0, 2.0, (3, V))
    tile[0, ::17] = np.nan
    tile[1, 5] = np.inf
    return tile


@pytest.mark.parametrize("E,H", [(1.0, 2.0), (0.5, 1.0)])
def test_renumbering_the_vertices_permutes_the_output_bit_for_bit(E, H):
    rng = np.random.default_rng(5)
    V = 200
    off, nbr = _random_graph(V, rng)
    tile = _noise(V, rng)
    w = rng.integers(0, 1 << 33, V)
    new_of_old = rng.permutation(V)
    off2, nbr2 = tref.relabel(off, nbr, new_of_old)
    tile2, w2 = np.empty_like(tile), np.empty_like(w)
    tile2[:, new_of_old], w2[new_of_old] = tile, w
    for weights, weights2 in ((None, None), (w, w2)):
        got, clip = tref.tfce(tile, off, nbr, dh=0.25, E=E, H=H, weights=weights, unit=2.0 ** -20, max_steps=40)
        got2, clip2 = tref.tfce(tile2, off2, nbr2, dh=0.25, E=E, H=H, weights=weights2, unit=2.0 ** -20, max_steps=40)
        same_bits(got2[:, new_of_old], got, "renumbered tfce")
        assert np.array_equal(clip, clip2) and clip.tolist() == [0, 1, 0]
        assert np.abs(got[2]).max() > 0


def test_flipping_the_sign_of_t_flips_the_sign_of_tfce_bit_for_bit():
    """Where t is not exactly zero: +0.0 and -0.0 both have side 0 and give +0.0."""
    rng = np.random.default_rng(6)
    V = 200
    off, nbr = _random_graph(V, rng)
    tile = _noise(V, rng)
    assert (tile != 0).all()
    got, clip = tref.tfce(tile, off, nbr, dh=0.1, max_steps=50)
    neg, clip_neg = tref.tfce(-tile, off, nbr, dh=0.1, max_steps=50)
    same_bits(neg, -got, "tfce of -t")
    assert np.array_equal(clip, clip_neg)
    assert (np.signbit(got) == np.signbit(tile))[~np.isnan(tile)].all()
    zeros, _ = tref.tfce(np.array([[0.0, -0.0, 0.05, -0.05]]), *tref.path_graph(4), dh=0.1)
    assert np.signbit(zeros[0]).tolist() == [False, False, False, True] and (zeros == 0).all()
