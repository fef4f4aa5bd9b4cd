"""Inputs for the radix select of csrc/radix_select.h built from bit patterns, so that the bin each of its four ranks falls in at each
pass is chosen: the order-preserving key of a float32 (key_of) and its inverse in numpy, numpy's float32 percentile index restated, and
arrays with given keys at the four ranks of a percentile pair."""
import numpy as np

FINITE_LO, FINITE_HI = 0x00800000, 0xFF7FFFFF          # keys of -FLT_MAX and +FLT_MAX
INF_LO, INF_HI = 0x007FFFFF, 0xFF800000                # keys of -inf and +inf; everything outside is a NaN
NEG_ZERO = 0x7FFFFFFF                                  # key of -0.0: below +0.0 on the device, unordered in numpy's sort -- kept out


def key_of(f):
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float_of(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def ranks(n, pct):
    """(k, k + 1 clamped, gamma) of np.percentile(a, pct) on n float32 values: the quantile, the virtual index and gamma in float32."""
    q = np.float32(pct) / np.float32(100)
    vi = np.float32(n - 1) * q
    fl = max(np.floor(vi), np.float32(0))
    k, gamma = int(fl), np.float32(vi - fl)
    if k >= n - 1:
        k, gamma = n - 1, np.float32(0)
    return k, min(k + 1, n - 1), gamma


def four_ranks(n, lo, hi):
    return ranks(n, lo)[:2] + ranks(n, hi)[:2]


def lerp(a, b, t):
    """numpy's _lerp in float32."""
    a, b, t = np.float32(a), np.float32(b), np.float32(t)
    with np.errstate(all="ignore"):
        d = np.float32(b - a)
        return np.float32(a + np.float32(d * t)) if t < np.float32(0.5) else np.float32(b - np.float32(d * np.float32(np.float32(1) - t)))


def first_diff_byte(a, b):
    """The pass (0 = most significant byte) at which two keys part; 4 if they are equal."""
    x = int(a) ^ int(b)
    return 4 if x == 0 else 3 - (x.bit_length() - 1) // 8


def _fill(rng, count, lo, hi):
    """``count`` keys in [lo, hi]: half at offsets of every magnitude above lo, half below hi, so that the neighbours of a rank share its
    prefix to every length; both ends are present from two keys on."""
    if count <= 0:
        return np.zeros(0, np.uint32)
    span = int(hi) - int(lo)
    assert span >= 0
    off = np.minimum((rng.random(count) * 2.0 ** rng.integers(0, 33, count)).astype(np.int64), span)
    up = np.arange(count) % 2 == 0
    keys = np.where(up, int(lo) + off, int(hi) - off)
    keys[:2] = (int(lo), int(hi))[:min(count, 2)]
    keys[keys == NEG_ZERO] = NEG_ZERO + 1 if hi > NEG_ZERO else NEG_ZERO - 1
    assert keys.min() >= lo and keys.max() <= hi
    return keys.astype(np.uint32)


def sorted_keys(n, lo_pct, hi_pct, keys4, seed, lo_key=FINITE_LO, hi_key=FINITE_HI):
    """n sorted keys with keys4[i] at the i-th of the four ranks of (lo_pct, hi_pct); the rest drawn between the neighbouring chosen
    keys, from lo_key below the first rank and up to hi_key above the last."""
    rng = np.random.default_rng(seed)
    want = {}
    for r, k in zip(four_ranks(n, lo_pct, hi_pct), keys4):
        assert want.setdefault(r, int(k)) == int(k), "one rank, two keys"
    rs = sorted(want)
    assert all(want[a] <= want[b] for a, b in zip(rs, rs[1:])) and lo_key <= want[rs[0]] and want[rs[-1]] <= hi_key
    parts = [_fill(rng, rs[0], lo_key, want[rs[0]])]
    for a, b in zip(rs, rs[1:] + [None]):
        parts.append(np.array([want[a]], np.uint32))
        parts.append(_fill(rng, (n if b is None else b) - a - 1, want[a], hi_key if b is None else want[b]))
    keys = np.concatenate(parts)
    assert keys.size == n and not (keys == NEG_ZERO).any()
    out = np.sort(keys)
    for r in rs:                                           # sorting moved no chosen key: every fill lies between its neighbours
        assert out[r] == want[r]
    return out
