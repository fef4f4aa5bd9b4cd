"""GPU: the decision tree of the 4-rank, 4-pass radix select (csrc/radix_select.h) through both of its owners: ops.image_normalize
(window values and windowed image against oracle.normalize.image_normalize, i.e. np.percentile) and ops.surface_distance (two
percentiles of the pooled, filtered distances against np.percentile).  Window values are compared as uint32 bit patterns; where the
reference is +-0 with ``==``, because numpy's sort does not order -0.0 and +0.0 (-0.0 is kept out of the inputs for the same reason).
NaN inputs are out of scope: numpy returns NaN and the device does not claim to, so no input here holds a NaN.

The arrays are built from bit patterns (tests/radix_select_ref.py): the keys at the four ranks k_lo, k_lo + 1, k_hi, k_hi + 1 are chosen,
the other elements are drawn between them at offsets of every magnitude (so that a rank's neighbours share its prefix to every length),
and the test asserts, before it runs the device, that the sorted array holds the chosen keys at the ranks of numpy's float32 index
arithmetic, that those keys part at the intended pass, and that np.percentile is numpy's lerp of exactly those two order statistics.
Byte p of a key is the bin at pass p.

  case                          what of radix_select.h it is there to catch
  share_bytes_0_2               all four ranks in row 0 for passes 0-2 (same01, same02, same23 all true; ``row`` 0 for ranks 1-3)
  part_at_p                     the lo pair and the hi pair part at pass p: from pass p + 1 on ``!same02`` counts row 2, rank 3 reads row 2
                                (``pre[3] == pre[2] ? (pre[2] == pre[0] ? 0 : 2)``), rank 1 still reads row 0
  lo_straddle_p_far / _near     k_lo | k_lo + 1 in two bins at pass p: ``!same01`` counts row 1 on its own; near: ranks 1, 2, 3 share a
                                prefix that rank 0 does not (rows 1 and 2 both counted, rank 3 reads row 2)
  hi_straddle_p_far / _near     k_hi | k_hi + 1 in two bins at pass p: ``!same23 && !(pre[3] == pre[0])`` counts row 3 on its own; near:
                                ranks 0, 1, 2 still share row 0 (``same02``) while rank 3 has left it
  adjacent_*                    ranks k, k+1, k+1, k+2: ranks 1 and 2 are one element; the boundary between k | k+1 (ranks 1, 2 share
                                a prefix without rank 0) and between k+1 | k+2 (rank 3 alone), n = 5 and n = 257
  bin255_pass_p (+inf)          a rank in bin 255: the ``d < 255`` fall-through of select_scan_step (bin 255 is never compared)
  bin0_pass_p (-inf)            a rank in bin 0: ``rem < c`` at d = 0, and key_of / float_of on negative values with the largest exponent
  denormals                     key_of / float_of around zero; no flush to zero in the select, the lerp or the window
  inf_present                   +-inf in the array with finite percentiles: keys 0x007fffff and 0xff800000 are counted like any other
  two_values*                   heavy ties: ``rem`` runs over bins holding hundreds of equal keys; the straddle puts k | k+1 on the two
  pct_0_100                     numpy_virtual_index: k = 0, and the ``k >= n - 1`` clamp with gamma = 0 (k_hi = k_hi + 1 = n - 1)
  n_2 / n_3 / n_4               the smallest arrays: ranks coincide, k + 1 clamps to n - 1
  n % 4 in {1, 2, 3}, n = 4096  the scalar tail of window_apply_kernel (most cases have n = 1003), and none
  mri_like at 160*384*384,      n > 2^24: (float)(n - 1) is rounded; the grid cap of 2048 blocks (n > 8.4 M); more than 2^23 equal values
  2^24 + 1, 2^24 + 3            in one bin (40 % exact zeros); 0.1 / 99.9, 0 / 100, 25 / 50

Percentiles within about 1e-5 of 100 (but not 100) are avoided at the large sizes: there np.percentile itself raises, its float32 index
rounds up to n."""
import functools

import numpy as np
import pytest
import torch

import radix_select_ref as rs
from oracle import normalize as onorm

pytestmark = pytest.mark.gpu


def K(b0, b1, b2, b3):
    return (b0 << 24) | (b1 << 16) | (b2 << 8) | b3


def _bump(key, p):
    """The key two bins higher at pass p."""
    return key + (2 << (24 - 8 * p))


# k and k + 1 of one percentile are GAP keys apart where they share bytes 0-2: numpy's lerp of two neighbouring floats rounds to one of
# them, and a wrong other one would go unseen; at weights 0.25, 0.5 and 0.75 a gap of four gives three values that depend on both
GAP = 4


LO, HI = K(0x41, 0x23, 0x45, 0x10), K(0xC1, 0x23, 0x45, 0x10)          # a negative and a positive value: they part at pass 0


def _cases():
    c = {}

    def add(name, keys4, expect, n=1003, pct=(25.0, 75.0), **kw):
        assert name not in c
        c[name] = dict(n=n, pct=pct, keys4=keys4, expect=expect, **kw)

    add("share_bytes_0_2", (HI, HI + 0x10, HI + 0x20, HI + 0x30), {(0, 1): 3, (1, 2): 3, (2, 3): 3})
    add("share_bytes_0_2_n4096", (HI, HI + 0x10, HI + 0x20, HI + 0x30), {(0, 1): 3, (1, 2): 3, (2, 3): 3}, n=4096, pct=(10.0, 61.0))
    for p in range(4):
        lo = LO if p == 0 else HI
        hi = HI if p == 0 else HI + (0x60 << (24 - 8 * p))
        add(f"part_at_{p}", (lo, lo + GAP, hi, hi + GAP), {(0, 1): 3, (1, 2): p, (2, 3): 3}, n=(1002, 1003, 1004, 1006)[p])
        add(f"lo_straddle_{p}_far", (LO, _bump(LO, p), HI, HI + GAP), {(0, 1): p, (1, 2): 0, (2, 3): 3})
        add(f"hi_straddle_{p}_far", (LO, LO + GAP, HI, _bump(HI, p)), {(0, 1): 3, (1, 2): 0, (2, 3): p})
        if p < 3:
            b = _bump(HI, p)
            add(f"lo_straddle_{p}_near", (HI, b, b + 0x10, b + 0x20), {(0, 1): p, (1, 2): 3, (2, 3): 3})
            add(f"hi_straddle_{p}_near", (HI, HI + 0x10, HI + 0x20, _bump(HI + 0x20, p)), {(0, 1): 3, (1, 2): 3, (2, 3): p})
    # ranks k, k+1, k+1, k+2 with both weights non-zero, so that all three order statistics reach the window: virtual indices 1.2 and
    # 2.2 of n = 5, 64.5 and 65.5 of n = 257 (100 * 64.5 / 256 and 100 * 65.5 / 256 are exact in float32)
    for tag, n, pct in (("n5", 5, (30.0, 55.0)), ("n257", 257, (25.1953125, 25.5859375))):
        add(f"adjacent_shared_{tag}", (HI, HI + 0x10, HI + 0x10, HI + 0x20), {(0, 1): 3, (1, 2): 4, (2, 3): 3}, n=n, pct=pct, adjacent=True)
        for p in range(3):
            b = _bump(HI, p)
            add(f"adjacent_k_k1_part_at_{p}_{tag}", (HI, b, b, b + 0x10), {(0, 1): p, (1, 2): 4, (2, 3): 3}, n=n, pct=pct, adjacent=True)
            add(f"adjacent_k1_k2_part_at_{p}_{tag}", (HI, HI + 0x10, HI + 0x10, _bump(HI + 0x10, p)), {(0, 1): 3, (1, 2): 4, (2, 3): p}, n=n, pct=pct,
                adjacent=True)
    big, small = K(0xFF, 0x12, 0x34, 0x56), K(0x00, 0xA0, 0x00, 0x00)                    # >= 2^127 and <= -2^127
    add("bin255_pass_0", (LO, LO + GAP, big, big + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={2: (0, 255), 3: (0, 255)})
    add("bin255_pass_0_inf", (LO, LO + GAP, big, big + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={2: (0, 255), 3: (0, 255)}, hi_key=rs.INF_HI, inf=True)
    add("bin0_pass_0", (small, small + GAP, HI, HI + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={0: (0, 0), 1: (0, 0)})
    add("bin0_pass_0_inf", (small, small + GAP, HI, HI + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={0: (0, 0), 1: (0, 0)}, lo_key=rs.INF_LO, inf=True)
    for p in (1, 2):
        top = HI | (0xFF << (24 - 8 * p))
        bot = LO & ~(0xFF << (24 - 8 * p))
        add(f"bin255_pass_{p}", (LO, LO + GAP, top, top + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={2: (p, 255), 3: (p, 255)})
        add(f"bin0_pass_{p}", (bot, bot + GAP, HI, HI + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={0: (p, 0), 1: (p, 0)})
    add("bin255_pass_3", (LO, LO + GAP, HI | 0xFB, HI | 0xFF), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={3: (3, 255)})
    add("bin255_pass_3_both", (LO | 0xFB, LO | 0xFF, HI | 0xFF, (HI | 0xFF) + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 2}, bins={1: (3, 255), 2: (3, 255)})
    add("bin0_pass_3", (LO & ~0xFF, (LO & ~0xFF) + GAP, HI, HI + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, bins={0: (3, 0)})
    nd, pd = K(0x7F, 0x9A, 0xBC, 0x10), K(0x80, 0x23, 0x45, 0x10)                        # a negative and a positive denormal
    add("denormals", (nd, nd + GAP, pd, pd + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, lo_key=0x7F800001, hi_key=0x807FFFFF, denormal=True)
    add("inf_present", (LO, LO + GAP, HI, HI + GAP), {(0, 1): 3, (1, 2): 0, (2, 3): 3}, lo_key=rs.INF_LO, hi_key=rs.INF_HI, inf=True, n=300)
    add("pct_0_100", (LO, LO + 0x100, HI, HI), {(0, 1): 2, (1, 2): 0, (2, 3): 4}, pct=(0.0, 100.0))
    add("pct_0_100_n4096", (LO, LO + 0x100, HI, HI), {(0, 1): 2, (1, 2): 0, (2, 3): 4}, pct=(0.0, 100.0), n=4096)
    v1, v2 = HI, _bump(HI, 1)
    c["two_values"] = dict(n=1000, pct=(25.0, 75.0), keys=[v1] * 400 + [v2] * 600, expect={(0, 1): 4, (1, 2): 1, (2, 3): 4})
    c["two_values_straddle"] = dict(n=1003, pct=(25.0, 75.0), keys=[v1] * 251 + [v2] * 752, expect={(0, 1): 1, (1, 2): 4, (2, 3): 4})
    few = [LO, K(0x80, 0, 0, 0), HI, _bump(HI, 2)]                                          # a negative value, +0.0, two positive ones
    for n in (2, 3, 4):
        for pct in ((0.0, 100.0), (25.0, 75.0)):
            c[f"n_{n}_pct_{int(pct[0])}_{int(pct[1])}"] = dict(n=n, pct=pct, keys=few[4 - n:], expect={})
    return c


CASES = _cases()
POOLED = [name for name in CASES if name.startswith(("part_at_", "lo_straddle_", "hi_straddle_", "adjacent_k", "bin255_pass_1", "two_values"))]


@functools.lru_cache(maxsize=None)
def _build(name):
    """(the shuffled float32 array, its sorted keys, the four ranks) of a case, with the construction asserted."""
    case = CASES[name]
    n, (lo, hi) = case["n"], case["pct"]
    seed = sorted(CASES).index(name)
    if "keys" in case:
        keys = np.sort(np.array(case["keys"], np.uint32))
    else:
        keys = rs.sorted_keys(n, lo, hi, case["keys4"], seed, case.get("lo_key", rs.FINITE_LO), case.get("hi_key", rs.FINITE_HI))
    assert keys.size == n and (keys >= rs.INF_LO).all() and (keys <= rs.INF_HI).all() and not (keys == rs.NEG_ZERO).any()      # no NaN, no -0.0
    r = rs.four_ranks(n, lo, hi)
    if "keys4" in case:
        assert tuple(int(keys[i]) for i in r) == tuple(case["keys4"])
    for pct in (lo, hi):                                                  # k and k + 1 both weigh in, save at the two ends
        assert pct in (0.0, 100.0) or 0 < rs.ranks(n, pct)[2] < 1, (name, pct)
    if case.get("adjacent"):
        assert r[1] == r[2] == r[0] + 1 and r[3] == r[0] + 2
    for (i, j), p in case["expect"].items():                              # the pass at which two ranks part company
        assert rs.first_diff_byte(keys[r[i]], keys[r[j]]) == p, (name, i, j)
    for i, (p, b) in case.get("bins", {}).items():                        # the bin a rank falls in at pass p
        assert (int(keys[r[i]]) >> (24 - 8 * p)) & 255 == b, (name, i)
    a = rs.float_of(keys)
    assert np.array_equal(rs.key_of(a), keys) and not np.isnan(a).any() and np.array_equal(np.sort(a), a)
    assert bool(np.isinf(a).any()) == bool(case.get("inf")) and (not case.get("inf") or (np.isinf(a[[0, -1]]).sum() >= 1))
    if case.get("denormal"):
        assert (np.abs(a) < np.finfo(np.float32).tiny).all() and (a[r[0]] < 0 < a[r[2]])
    with np.errstate(all="ignore"):
        for pct, (i, j) in ((lo, (0, 1)), (hi, (2, 3))):                  # the ranks are numpy's: its percentile is the lerp of these two
            want, mine = np.float32(np.percentile(a, pct)), rs.lerp(a[r[i]], a[r[j]], rs.ranks(n, pct)[2])
            assert np.isfinite(want) and _same_bits(mine, want), (name, pct)
            if 0 < rs.ranks(n, pct)[2] < 1 and a[r[i]] != a[r[j]]:           # ... and shows a wrong one of either
                assert a[r[i]] < want < a[r[j]], (name, pct)
    shuffled = a.copy()
    np.random.default_rng(seed).shuffle(shuffled)
    return shuffled, keys, r


def _same_bits(got, want):
    got, want = np.float32(got), np.float32(want)
    return bool(got == want) if want == 0 else bool(got.view(np.uint32) == want.view(np.uint32))


def _check_normalize(a, lo, hi, x=None, label=""):
    from oai_analysis_2_amd import ops
    with np.errstate(all="ignore"):
        ref, (wmin, wmax) = onorm.image_normalize(a, lo, hi, 0, 1)
    assert wmin < wmax
    got, win = ops.image_normalize(torch.from_numpy(a).cuda() if x is None else x, lo, hi, 0, 1, return_window=True)
    win = win.cpu().numpy()
    print(label, "window", win.view(np.uint32), "reference", np.array([wmin, wmax], np.float32).view(np.uint32))
    assert _same_bits(win[0], wmin) and _same_bits(win[1], wmax), label
    assert np.array_equal(got.cpu().numpy(), ref), label


@pytest.mark.parametrize("name", list(CASES))
def test_image_normalize_on_chosen_bit_patterns(name):
    a, _, _ = _build(name)
    _check_normalize(a, *CASES[name]["pct"], label=name)


@pytest.mark.parametrize("name", POOLED)
def test_surface_distance_percentiles_on_chosen_bit_patterns(name):
    """The same select behind its second owner: the ranks come from the count of a filtered stream pooled from two arrays, and every
    element that the masks leave out is a decoy drawn from the same values."""
    from oai_analysis_2_amd import ops
    a, _, _ = _build(name)
    lo, hi = CASES[name]["pct"]
    n = a.size
    rng = np.random.default_rng(n)
    length, n_a = n + 37, max(n // 3, 1)
    sa, sb = np.zeros(length, np.uint8), np.zeros(length, np.uint8)
    sa[rng.choice(length, n_a, replace=False)] = 1
    sb[rng.choice(length, n - n_a, replace=False)] = 1
    db, da = rng.choice(a, length), rng.choice(a, length)
    db[sa != 0], da[sb != 0] = a[:n_a], a[n_a:]
    pooled = np.concatenate([db[sa != 0], da[sb != 0]])
    assert np.array_equal(np.sort(pooled), np.sort(a))
    dev4 = tuple(torch.from_numpy(t).cuda() for t in (sa, db, sb, da))
    with np.errstate(all="ignore"):
        want = [np.float32(np.percentile(pooled, q)) for q in (lo, hi)]
    s = ops.surface_distance(*dev4, (lo, hi)).cpu().numpy()
    assert (s[0], s[1]) == (n_a, n - n_a)
    for i in (0, 1):
        assert np.float32(s[6 + i]) == s[6 + i] and _same_bits(s[6 + i], want[i]), (name, i)
    one = ops.surface_distance(*dev4, (lo,)).cpu().numpy()                 # one percentile: ranks 2 and 3 are copies of rank 0
    assert _same_bits(one[6], want[0]) and np.isnan(one[7])


# ---- production sizes ------------------------------------------------------------------------------------------------------------------
LARGE_N = [160 * 384 * 384, 2 ** 24 + 1, 2 ** 24 + 3]


@functools.lru_cache(maxsize=1)                                           # one size at a time, on the host and on the device
def _mri_like(n):
    rng = np.random.default_rng(5)
    a = rng.gamma(2.0, 150.0, n).astype(np.float32)                       # a long intensity tail ...
    a[rng.random(n) < 0.4] = 0.0                                          # ... over a large background of exact zeros
    return a, torch.from_numpy(a).cuda()


@pytest.mark.parametrize("pct", [(0.1, 99.9), (0.0, 100.0), (25.0, 50.0)])
@pytest.mark.parametrize("n", LARGE_N)
def test_image_normalize_above_2_to_24(n, pct):
    a, x = _mri_like(n)
    assert n > 2 ** 24 and (n + 4095) // 4096 > 2048 and int((a == 0).sum()) > 2 ** 22
    if n == LARGE_N[0]:
        assert int((a == 0).sum()) > 2 ** 23
    _check_normalize(a, *pct, x=x, label=(n, pct))
