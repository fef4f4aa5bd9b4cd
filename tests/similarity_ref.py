"""A numpy restatement of csrc/similarity.hip, operation for operation in fp64 (float32 where the kernel works in float32): the
filter as pad-and-shifted-slices with ``acc = acc + w[j] * p[...]``, the float32 binning rule, the entropies and the moments.  IEEE
add, multiply, divide and sqrt on numpy float64 are bit-faithful, and the reductions go through tests/ordered_reduce_ref.py in the
order the kernels take, so the device's figures are expected to equal these bit for bit (the entropies up to the device's log)."""
import numpy as np

import ordered_reduce_ref as orr

KT = orr.KT
MOMENT_BLOCKS = 2048                       # kStreamBlocks
MOM_OPS = ("add",) * 8
MOM_CLEAR = np.zeros(8)
LNCC_OPS = ("add", "add", "add", "add", "min", "max")
LNCC_CLEAR = np.array([0.0, 0.0, 0.0, 0.0, np.inf, -np.inf])
ENT_OPS = ("add", "add", "add")


def gaussian_taps(sigma):
    """ops.gaussian_taps, restated."""
    sigma = float(sigma)
    if not sigma > 0.0:
        return np.ones(1, np.float64), 0
    radius = int(2.0 * sigma)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum(), radius


# ---- the filter and the map ---------------------------------------------------------------------------------------------------------------
def filter_axis(v, taps, radius, axis):
    """acc = 0; for j ascending: acc = acc + taps[j] * v[reflect(i + j - radius)] along ``axis`` (np.pad's "reflect")."""
    n = v.shape[axis]
    if not n > radius:
        raise ValueError(f"axis {axis} of length {n} is not longer than the radius {radius}")
    pad = [(0, 0)] * v.ndim
    pad[axis] = (radius, radius)
    p = np.pad(v, pad, mode="reflect")
    acc = np.zeros_like(v, dtype=np.float64)
    for j in range(2 * radius + 1):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(j, j + n)
        acc = acc + taps[j] * p[tuple(sl)]
    return acc


def filter3(v, taps, radius):
    """x, then y, then z of a [z,y,x] volume."""
    for axis in (2, 1, 0):
        v = filter_axis(v, taps, radius, axis)
    return v


def lncc_map(a, b, taps, radius, eps=1e-5):
    """The fp64 map of cc of two float32 [z,y,x] volumes."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Ea, Eb, Eaa, Ebb, Eab = (filter3(c, taps, radius) for c in (a, b, a * a, b * b, a * b))
        cov = Eab - Ea * Eb
        va = Eaa - Ea * Ea
        vb = Ebb - Eb * Eb
        return cov / np.sqrt((va + eps) * (vb + eps))


def lncc_stats(cc, mask=None):
    """stats[0..5] of oai_lncc from a map of cc: one voxel per thread, block k = voxels [256 k, 256 k + 256), then the finish."""
    cc = np.asarray(cc, np.float64).reshape(-1)
    n = cc.size
    nb = -(-n // KT)
    acc = np.tile(LNCC_CLEAR, (nb * KT, 1))
    on = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    good = on & np.isfinite(cc)
    idx = np.flatnonzero(good)
    v = cc[idx]
    acc[idx, 0] = acc[idx, 0] + 1.0
    acc[idx, 2] = acc[idx, 2] + v
    acc[idx, 3] = acc[idx, 3] + v * v
    acc[idx, 4] = np.fmin(acc[idx, 4], v)
    acc[idx, 5] = np.fmax(acc[idx, 5], v)
    bad = np.flatnonzero(on & ~np.isfinite(cc))
    acc[bad, 1] = acc[bad, 1] + 1.0
    s = orr.finish(orr.block_reduce(acc.reshape(nb, KT, 6), LNCC_OPS), LNCC_CLEAR, LNCC_OPS)
    if not s[0] > 0:
        s[4] = s[5] = np.nan
    return s


# ---- the moments --------------------------------------------------------------------------------------------------------------------------
def moment_blocks(n):
    return min(MOMENT_BLOCKS, -(-n // (4 * KT)))


def moments_stats(a, b, mask=None):
    """stats[0..7] of oai_image_moments: thread g of moment_blocks(n) blocks adds positions g, g + threads, ... in that order."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    n = a.size
    blocks = moment_blocks(n)
    if blocks == 0:
        return orr.finish(np.zeros((0, 8)), MOM_CLEAR, MOM_OPS)
    threads = blocks * KT
    on = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    acc = np.tile(MOM_CLEAR, (threads, 1))
    for start in range(0, n, threads):
        m = min(threads, n - start)
        sa, sb, so = a[start:start + m], b[start:start + m], on[start:start + m]
        fin = np.isfinite(sa) & np.isfinite(sb)
        g = np.flatnonzero(so & fin)
        da, db = sa[g].astype(np.float64), sb[g].astype(np.float64)
        d = da - db
        for k, term in ((0, 1.0), (2, da), (3, db), (4, da * da), (5, db * db), (6, da * db), (7, d * d)):
            acc[g, k] = acc[g, k] + term
        bad = np.flatnonzero(so & ~fin)
        acc[bad, 1] = acc[bad, 1] + 1.0
    return orr.finish(orr.block_reduce(acc.reshape(blocks, KT, 8), MOM_OPS), MOM_CLEAR, MOM_OPS)


def ncc_mse(stats):
    """qc.ncc_from_moments, restated: Pearson's r and the mean squared error from the eight doubles."""
    n, _, sa, sb, saa, sbb, sab, sdd = (float(v) for v in stats)
    if n <= 0:
        return float("nan"), float("nan")
    cov, va, vb = sab / n - (sa / n) * (sb / n), saa / n - (sa / n) ** 2, sbb / n - (sb / n) ** 2
    return (cov / np.sqrt(va * vb) if va > 0 and vb > 0 else float("nan")), sdd / n


# ---- the histogram and its entropies ------------------------------------------------------------------------------------------------------
def bin_of(x, lo, hi, bins):
    """min((int)((clamp(x, lo, hi) - lo) * scale), bins - 1) in float32, scale = float32(bins / (double(hi) - double(lo))); x finite."""
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(bins / (float(hi) - float(lo)))
    c = np.minimum(np.maximum(np.asarray(x, np.float32), lo), hi)
    k = ((c - lo) * scale).astype(np.int32)
    return np.minimum(k, bins - 1)


def joint_histogram(a, b, bins, range_a=(0.0, 1.0), range_b=(0.0, 1.0), mask=None):
    """int64 [bins*bins + 1]: the table, and the admitted positions skipped for a non-finite value."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    on = np.ones(a.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    fin = np.isfinite(a) & np.isfinite(b)
    g = on & fin
    cell = bin_of(a[g], *range_a, bins).astype(np.int64) * bins + bin_of(b[g], *range_b, bins)
    hist = np.zeros(bins * bins + 1, np.int64)
    hist[:bins * bins] = np.bincount(cell, minlength=bins * bins)
    hist[-1] = int((on & ~fin).sum())
    return hist


def _plogp_runs(counts, total):
    """[KT] per-thread sums of p log p over the non-zero entries of ``counts``: thread t takes its run of consecutive cells in order."""
    cells = counts.size
    per = -(-cells // KT)
    acc = np.zeros(KT)
    for j in range(per):
        idx = np.arange(KT) * per + j
        ok = idx < cells
        c = np.where(ok, counts[np.minimum(idx, cells - 1)], 0)
        nz = c > 0
        p = c[nz].astype(np.float64) / total
        acc[nz] = acc[nz] + p * np.log(p)
    return acc


def entropies(hist, bins):
    """out[0..3] of oai_histogram_entropies: N, H_A, H_B, H_AB."""
    table = np.asarray(hist, np.int64)[:bins * bins].reshape(bins, bins)
    count = int(table.sum())
    if count == 0:
        return np.array([0.0, np.nan, np.nan, np.nan])
    total = float(count)
    acc = np.stack([_plogp_runs(table.sum(axis=1), total), _plogp_runs(table.sum(axis=0), total), _plogp_runs(table.reshape(-1), total)], axis=-1)
    return np.concatenate([[total], 0.0 - orr.block_reduce(acc, ENT_OPS)])


def mi_nmi(ent):
    """qc's host arithmetic: mi = H_A + H_B - H_AB, nmi = (H_A + H_B) / H_AB (Studholme)."""
    _, ha, hb, hab = (float(v) for v in ent)
    return ha + hb - hab, ((ha + hb) / hab if hab > 0 else float("nan"))
