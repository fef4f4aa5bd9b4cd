"""CPU: the helpers of tests/cohort_cases.py that every "equal to the bit" of the cohort tests rests on -- ``same_bits`` passes what is
equal and refuses one ulp, the sign of a zero, a NaN against a number, another dtype and another shape; ``same_result`` refuses a missing
key, an extra key and 1 against 1.0 -- and the icosphere that the end-to-end tests stand on."""
import dataclasses

import numpy as np
import pytest
import torch

from cohort_cases import icosphere, same_bits, same_result

FLOATS = (np.float32, np.float64)


def _values(dtype):
    """A few of everything: ordinary numbers, both zeros, an infinity, the smallest subnormal, two NaNs."""
    a = np.array([[1.5, -2.25, 0.0, -0.0], [np.inf, 3.0, np.nan, np.nan]], dtype)
    a[1, 1] = np.nextafter(dtype(0), dtype(1))
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64, np.uint8])
def test_equal_arrays_pass_as_arrays_and_as_tensors(dtype):
    a = _values(dtype) if dtype in FLOATS else np.arange(12, dtype=dtype).reshape(3, 4)
    same_bits(a.copy(), a, "array")
    same_bits(torch.from_numpy(a.copy()), a, "tensor")


@pytest.mark.parametrize("dtype", FLOATS)
def test_nans_of_another_payload_in_the_same_places_pass(dtype):
    as_int = np.int32 if dtype == np.float32 else np.int64
    a, b = _values(dtype), _values(dtype)
    b.view(as_int)[1, 2] ^= 5                                              # still a NaN, with other payload bits
    b[1, 3] = -np.nan                                                      # and one with the sign bit set
    assert np.isnan(b[1, 2:]).all() and (a.view(as_int)[1, 2:] != b.view(as_int)[1, 2:]).all()
    same_bits(b, a, "payloads")


@pytest.mark.parametrize("dtype", FLOATS)
def test_one_ulp_a_zeros_sign_and_a_nan_against_a_number_are_refused(dtype):
    a = _values(dtype)
    ulp = a.copy()
    ulp[0, 1] = np.nextafter(a[0, 1], dtype(0))
    zero = a.copy()
    zero[0, 2], zero[0, 3] = -0.0, 0.0                                     # equal by value at both places
    assert np.array_equal(zero, a, equal_nan=True)
    nan = a.copy()
    nan[0, 0] = np.nan
    number = a.copy()
    number[1, 2] = 0.0                                                     # what a NaN is replaced by before the bits are compared
    for other, words in ((ulp, ("1 of 8 differ", "first at [0, 1]")), (zero, ("2 of 8 differ", "first at [0, 2]")),
                         (nan, ("NaN positions differ",)), (number, ("NaN positions differ",))):
        for got, want in ((other, a), (a, other)):
            with pytest.raises(AssertionError) as failure:
                same_bits(got, want, "the label")
            assert "the label" in str(failure.value) and all(w in str(failure.value) for w in words), str(failure.value)


def test_another_dtype_another_shape_and_one_other_integer_are_refused():
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    for other in (a.astype(np.int64), a.astype(np.float32), a.reshape(4, 3), a[:2], a.reshape(-1)):
        with pytest.raises(AssertionError) as failure:
            same_bits(other, a, "the label")
        assert "the label" in str(failure.value) and str(other.dtype) in str(failure.value) and str(other.shape) in str(failure.value)
    for dtype in FLOATS:                                                   # equal values, other widths
        with pytest.raises(AssertionError):
            same_bits(_values(np.float32).astype(dtype), _values(np.float32).astype(FLOATS[dtype == np.float32]), "width")
    b = a.copy()
    b[2, 1] += 1
    with pytest.raises(AssertionError, match=r"the label: 1 of 12 differ, first at \[2, 1\]"):
        same_bits(torch.from_numpy(b), a, "the label")


@dataclasses.dataclass
class _Result:
    t: np.ndarray
    n: int
    exact: bool
    note: object = None


def test_same_result_wants_every_field_once_and_scalars_of_the_same_type():
    t = _values(np.float64)
    res = _Result(t.copy(), 1, False)
    res.n_dropped = np.arange(3)                                           # an attribute that is not a field
    want = dict(t=t, n=1, exact=False, note=None)
    same_result(res, want, "all fields")
    same_result(res, dict(want, n_dropped=np.arange(3)), "and an attribute", extra=("n_dropped",))
    for bad, words in (({k: v for k, v in want.items() if k != "note"}, "note"), (dict(want, p=0.5), "'p'"), (dict(want, n_dropped=np.arange(3)), "n_dropped"),
                       (dict(want, n=1.0), "n: 1 != 1.0"), (dict(want, exact=0), "exact: False != 0"), (dict(want, n=2), "n: 1 != 2"),
                       (dict(want, t=-t), "the label: t: ")):
        with pytest.raises(AssertionError) as failure:
            same_result(res, bad, "the label")
        assert "the label" in str(failure.value) and words in str(failure.value), str(failure.value)
    with pytest.raises(AssertionError, match="n_dropped"):
        same_result(res, want, "the label", extra=("n_dropped",))


def test_the_icosphere_of_level_3_is_a_closed_unit_sphere_and_read_only():
    verts, faces = icosphere(3)
    assert verts.shape == (642, 3) and verts.dtype == np.float32 and faces.shape == (1280, 3) and faces.dtype == np.int32
    assert np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    _, count = np.unique(edges, axis=0, return_counts=True)
    assert len(count) == 1920 and (count == 2).all() and sorted(np.unique(faces).tolist()) == list(range(642))
    assert icosphere(3)[0] is verts and not verts.flags.writeable and not faces.flags.writeable
    assert all(np.array_equal(a, b) for a, b in zip(icosphere(), icosphere(3)))                        # the default level
