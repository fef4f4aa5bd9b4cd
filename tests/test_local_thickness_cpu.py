"""CPU: the restatement of the thickness QC (tests/local_thickness_ref.py; include/oai_hip.h, "Thickness QC") -- the brute force over
all pairs and the loop over offsets agree to the bit, the slab law of the voxel radius, the definition against scipy's transform, the
cap rule and the window, the restated statistics -- and the argument checks of the new entry points, which touch no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import edt_ref as er
import local_thickness_ref as lt


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", er.SHAPES_SMALL)
def test_the_two_forms_agree_to_the_bit(shape, spacing):
    for name, field in (("edt", lt.edt_field(shape, spacing, seed=11)), ("generic", lt.generic_field(shape, spacing, seed=12))):
        brute, offsets = lt.sq_brute(field, spacing), lt.sq_offsets(field, spacing)
        c = lt.centres(field)
        assert c.any() and not c.all(), name
        assert np.array_equal(_bits(brute), _bits(offsets)), (name, shape, spacing)
        assert (brute[c] >= field[c]).all() and (brute[~c] == 0.0).all()           # p covers itself; nothing off the centres
        assert np.isin(brute[c], field[c]).all()                                   # a max of the field's own entries: nothing is computed
    generic = lt.generic_field(shape, spacing, seed=12)
    for bad in (np.isnan(generic), np.isposinf(generic), np.isneginf(generic), generic < 0, generic == 0):
        assert bad.any() and not lt.centres(generic)[bad].any()


@pytest.mark.parametrize("spacing", er.SPACINGS)
def test_slab_law_of_the_voxel_radius(spacing):
    """A slab t voxels thick along z reads 2 ceil(t / 2) s_z at every voxel: sq == fl((ceil(t / 2) s_z)^2)."""
    sz = np.float64(spacing[2])
    for t in range(1, 7):
        m = lt.slab((t + 4, 5, 6), t)
        field = er.edt_sq_lines(~er.in_set(m), spacing)
        sq = lt.sq_brute(field, spacing)
        want = (np.float64(math.ceil(t / 2)) * sz) ** 2
        assert np.array_equal(_bits(sq[m > 0]), _bits(np.full(int((m > 0).sum()), want))), (t, spacing)
        assert (sq[m == 0] == 0.0).all()
        thick = lt.thickness32(sq)[m > 0]
        assert (thick >= np.float32(t * sz) * np.float32(1 - 1e-6)).all() and (thick <= np.float32((t + 1) * sz) * np.float32(1 + 1e-6)).all()


def test_against_scipy_on_one_shape():
    """scipy's transform, squared, is the canonical field to within 1e-12 relative and not to the bit (sqrt(5)^2 is 5.000000000000001),
    and the thickness from it cannot be compared voxel by voxel: the voxel opposite a centre's nearest background voxel sits at
    d2 == rsq exactly, the strict inequality leaves it out, and a last-bit growth of rsq takes it in.  The maximum is monotone in the
    field, so the definition on scipy's field lies between the definition on the canonical field shrunk and grown by 1e-12."""
    ndi = pytest.importorskip("scipy.ndimage")
    shape, eps = (9, 14, 17), 1e-12
    inside = er.in_set(er.blobs(shape, 11, tuple(n // 3 for n in shape)))
    for spacing in er.SPACINGS:
        d = ndi.distance_transform_edt(inside, sampling=spacing[::-1])
        field = lt.edt_field(shape, spacing, 11)
        assert np.allclose(d * d, field, rtol=eps, atol=0.0)
        got = lt.sq_brute(d * d, spacing)
        low, high = lt.sq_brute(field * (1.0 - eps), spacing), lt.sq_brute(field * (1.0 + eps), spacing)
        assert (low * (1.0 - eps) <= got).all() and (got <= high * (1.0 + eps)).all() and (low > 0).any()


def test_cap_rule_and_windows():
    spacing = (1.0, 1.0, 1.0)
    field = er.edt_sq_lines(~er.in_set(er.box((12, 12, 12), (2, 2, 2), (8, 8, 8))), spacing)
    vol = lt.windows(field, spacing)
    assert vol[0, 0, 0] == 0 and vol[2, 2, 2] == 1                 # off the set; a corner voxel at distance 1: k = 0 only (strict)
    assert vol[5, 5, 5] == 7 ** 3                                  # distance 4: k <= 3
    cap = lt.capped(field, spacing, 27)
    assert cap[5, 5, 5] and not cap[3, 3, 3] and not cap[2, 2, 2] and int(cap.sum()) == 4 ** 3
    free, held = lt.sq_offsets(field, spacing), lt.sq_offsets(field, spacing, 27)
    assert (held <= free).all() and (held < free).any() and (held[lt.centres(field)] >= field[lt.centres(field)]).all()
    assert np.array_equal(_bits(lt.sq_offsets(field, spacing, 7 ** 3)), _bits(free))
    wide = lt.windows(field, spacing, extra=1)
    assert (wide >= vol).all() and wide[5, 5, 5] == 9 ** 3


def test_restated_statistics():
    rng = np.random.default_rng(3)
    v = rng.normal(size=3000).astype(np.float32)
    v[[5, 17]] = np.nan, np.inf
    mask = (rng.uniform(size=3000) < 0.4).astype(np.uint8)
    mask[[5, 17]] = 1
    out = lt.masked_stats(v, mask, (50.0, 95.0))
    on = v[(mask != 0) & np.isfinite(v)]
    assert out[0] == on.size and out[7] == 2 and out[3] == on.min() and out[4] == on.max()
    assert out[5] == np.percentile(on, 50.0) and out[6] == np.percentile(on, 95.0)
    assert math.isclose(out[1], math.fsum(on.astype(np.float64)), rel_tol=1e-12, abs_tol=1e-9)
    assert math.isclose(out[2], math.fsum(on.astype(np.float64) ** 2), rel_tol=1e-12)
    empty = lt.masked_stats(v, np.zeros(3000, np.uint8))
    assert empty[0] == 0 and empty[7] == 0 and np.isnan(empty[1:7]).all()
    assert np.isnan(lt.masked_stats(np.zeros(0, np.float32))[1:7]).all()


def test_argument_checks_of_the_thickness_entry_points():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    dummy = (C.c_double * 8)()
    big = 1 << 30
    sp = lambda *v: (C.c_double * 3)(*v)
    err = lib.oai_last_error
    call = lambda rsq=dummy, dims=(2, 3, 4), s=sp(1, 1, 1), cap=64, thick=dummy, ws=dummy, nws=big: lib.oai_local_thickness(
        rsq, *dims, s, cap, None, thick, ws, nws, None, None)
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (32768, 2, 2), (2, 32768, 2), (2, 2, 32768), (2048, 2048, 512)):
        assert call(dims=dims) != 0 and b"every axis" in err()
        assert lib.oai_local_thickness_workspace_bytes(*dims) == 0
    need = lib.oai_local_thickness_workspace_bytes(2, 3, 4)
    assert need >= 17 * 24 and lib.oai_local_thickness_workspace_bytes(32767, 1, 1) > 0
    for kw in (dict(rsq=None), dict(thick=None), dict(ws=None), dict(s=None)):
        assert call(**kw) != 0 and b"null" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for c in range(3):
            v = [1.0, 1.0, 1.0]
            v[c] = bad
            assert call(s=sp(*v)) != 0 and b"spacing" in err()
    for cap in (0, -1):
        assert call(cap=cap) != 0 and b"max_window_voxels" in err()
    assert call(nws=need - 1) != 0 and b"oai_local_thickness: workspace" in err()

    pct = lambda *v: (C.c_float * 2)(*v)
    stats = lambda values=dummy, mask=dummy, n=8, p=pct(50, 95), k=2, ws=dummy, nws=big, out=dummy: lib.oai_masked_stats(
        values, mask, n, p, k, ws, nws, out, None)
    for kw in (dict(values=None), dict(ws=None), dict(out=None), dict(p=None)):
        assert stats(**kw) != 0 and b"null" in err()
    assert stats(n=-1) != 0 and b"negative" in err()
    for k in (3, -1):
        assert stats(k=k) != 0 and b"percentiles" in err()
    for bad in (-0.5, 100.5, float("nan")):
        assert stats(p=pct(50, bad)) != 0 and b"outside" in err()
    need = lib.oai_masked_stats_workspace_bytes(8)
    assert need > 0 and lib.oai_masked_stats_workspace_bytes(-1) == 0
    assert lib.oai_masked_stats_workspace_bytes(384 * 384 * 160) == lib.oai_masked_stats_workspace_bytes(1 << 40)      # the grid is capped
    assert stats(nws=need - 1) != 0 and b"oai_masked_stats: workspace" in err()
