"""numpy restatement of csrc/local_thickness.hip (include/oai_hip.h, "Thickness QC"): the local thickness of a squared-radius field as
the brute force over all pairs (the definition) and as a loop over offsets, the window of a centre and the cap rule, and the figures of
oai_masked_stats on tests/ordered_reduce_ref.py and np.percentile; with the seeded inputs the CPU and GPU tests share.  Not collected
as a test."""
import numpy as np

import edt_ref
import ordered_reduce_ref as orr

EXTRA_SHAPES = [(1, 1, 1), (1, 5, 7), (3, 4, 300), (5, 300, 4)]      # one voxel; a plane; x far beyond a wave; y long, x short
DESS = edt_ref.SPACINGS[1]


def centres(rsq):
    """A voxel is a centre when its squared radius is finite and > 0 (NaN, +-inf, zero and negative entries are not)."""
    rsq = np.asarray(rsq, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(rsq) & (rsq > 0.0)


def thickness32(sq):
    """thick = 2.0f * (float)sqrt(sq)."""
    return np.float32(2.0) * np.sqrt(np.asarray(sq, np.float64)).astype(np.float32)


def sq_brute(rsq, spacing_xyz, chunk=256):
    """sq_out[p] = max over the centres q with d2(p, q) < rsq[q] of rsq[q], d2 = (tx*tx + ty*ty) + tz*tz in fp64, over ALL pairs of
    centres: the definition.  0 where p is not a centre."""
    rsq = np.asarray(rsq, np.float64)
    sx, sy, sz = (np.float64(v) for v in spacing_xyz)
    c = np.argwhere(centres(rsq))                                  # [m, 3] (z, y, x): p and q both run over it
    r = rsq[tuple(c.T)]
    best = np.zeros(len(c))
    for i in range(0, len(c), chunk):
        q, rq = c[i:i + chunk], r[i:i + chunk]
        tx = (c[:, None, 2] - q[None, :, 2]).astype(np.float64) * sx
        ty = (c[:, None, 1] - q[None, :, 1]).astype(np.float64) * sy
        tz = (c[:, None, 0] - q[None, :, 0]).astype(np.float64) * sz
        d2 = (tx * tx + ty * ty) + tz * tz
        best = np.maximum(best, np.where(d2 < rq[None, :], rq[None, :], 0.0).max(axis=1))
    out = np.zeros(rsq.shape)
    out[tuple(c.T)] = best
    return out


def half_extents(rsq, spacing_xyz, extra=0):
    """Per voxel and axis (x, y, z) the largest k with fl((k s)^2) < rsq, limited to the axis (n - 1): the exact half-extent of the
    ball's bounding window; ``extra`` voxels are added before the limit.  Meaningless off the centres."""
    rsq = np.asarray(rsq, np.float64)
    D, H, W = rsq.shape
    r = np.where(centres(rsq), rsq, 1.0)
    out = []
    for s, n in zip(spacing_xyz, (W, H, D)):
        t = np.arange(n, dtype=np.float64) * np.float64(s)
        k = np.searchsorted(t * t, r.ravel(), side="left").reshape(r.shape) - 1        # the terms grow with k; k = 0 always passes
        out.append(np.minimum(k + extra, n - 1))
    return out


def windows(rsq, spacing_xyz, extra=0):
    """Per voxel the volume of its clipped window (int64 [D, H, W]); 0 off the centres."""
    rsq = np.asarray(rsq, np.float64)
    D, H, W = rsq.shape
    hx, hy, hz = half_extents(rsq, spacing_xyz, extra)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    vol = np.ones(rsq.shape, np.int64)
    for p, h, n in ((x, hx, W), (y, hy, H), (z, hz, D)):
        vol *= np.minimum(p + h, n - 1) - np.maximum(p - h, 0) + 1
    return np.where(centres(rsq), vol, 0)


def capped(rsq, spacing_xyz, max_window_voxels):
    """The centres whose clipped window holds more than ``max_window_voxels`` voxels: they cover only themselves."""
    return windows(rsq, spacing_xyz) > int(max_window_voxels)


def sq_offsets(rsq, spacing_xyz, max_window_voxels=None):
    """The same maximum as a loop over the offsets o = p - q: for each one the whole volume at once.  An offset whose d2 is not below
    the largest squared radius is skipped.  ``max_window_voxels``: the cap rule -- a capped centre takes part at o = 0 only."""
    rsq = np.asarray(rsq, np.float64)
    D, H, W = rsq.shape
    sx, sy, sz = (np.float64(v) for v in spacing_xyz)
    c = centres(rsq)
    r = np.where(c, rsq, 0.0)
    out = r.copy()                                                 # o = 0: every centre covers itself
    if not c.any():
        return out
    far = r if max_window_voxels is None else np.where(capped(rsq, spacing_xyz, max_window_voxels), 0.0, r)      # who reaches beyond itself
    rmax = far.max()
    hx, hy, hz = (int(np.where(c, h, 0).max()) for h in half_extents(rsq, spacing_xyz))
    for oz in range(-hz, hz + 1):
        tz = np.float64(oz) * sz
        for oy in range(-hy, hy + 1):
            ty = np.float64(oy) * sy
            for ox in range(-hx, hx + 1):
                tx = np.float64(ox) * sx
                d2 = (tx * tx + ty * ty) + tz * tz
                if (ox == 0 and oy == 0 and oz == 0) or not d2 < rmax:
                    continue
                # p = q + o: the voxels p in [lo, hi) per axis have their q inside the volume
                pz, py, px = (slice(max(o, 0), n + min(o, 0)) for o, n in ((oz, D), (oy, H), (ox, W)))
                qz, qy, qx = (slice(max(-o, 0), n + min(-o, 0)) for o, n in ((oz, D), (oy, H), (ox, W)))
                rq = far[qz, qy, qx]
                cand = np.where((d2 < rq) & c[pz, py, px], rq, 0.0)
                np.maximum(out[pz, py, px], cand, out=out[pz, py, px])
    return out


# ---- oai_masked_stats --------------------------------------------------------------------------------------------------------------------
MASKED_OPS = ("add", "add", "add", "min", "max", "add")            # n, sum v, sum v^2, min, max, non-finite
MASKED_CLEAR = np.array([0.0, 0.0, 0.0, np.inf, -np.inf, 0.0])


def masked_stats(values, mask=None, percentiles=(50.0, 95.0)):
    """out[0..7] of oai_masked_stats driven the way masked_partials_kernel is: blocks = min(2048, ceil(n / 1024)), thread b 256 + t
    takes i = b 256 + t, + blocks 256, ... in that order; each term is (double)float32, the square formed in fp64; the blocks' slots
    through ordered_reduce_ref.finish.  The percentiles are np.percentile of the counted float32 values."""
    v = np.asarray(values, np.float32).ravel()
    n = v.size
    on = np.ones(n, bool) if mask is None else np.asarray(mask).ravel() != 0
    fin = np.isfinite(v)
    out = np.full(8, np.nan)
    blocks = max(1, min(orr.STREAM_BLOCKS, -(-n // (4 * orr.KT)))) if n else 0
    threads = blocks * orr.KT
    acc = np.tile(MASKED_CLEAR, (max(threads, 1), 1))
    for start in range(0, n, max(threads, 1)):
        m = min(threads, n - start)
        good = np.flatnonzero(on[start:start + m] & fin[start:start + m])
        bad = np.flatnonzero(on[start:start + m] & ~fin[start:start + m])
        d = v[start:start + m][good].astype(np.float64)
        acc[good, 0] = acc[good, 0] + 1.0
        acc[good, 1] = acc[good, 1] + d
        acc[good, 2] = acc[good, 2] + d * d
        acc[good, 3] = np.fmin(acc[good, 3], d)
        acc[good, 4] = np.fmax(acc[good, 4], d)
        acc[bad, 5] = acc[bad, 5] + 1.0
    if blocks:
        tot = orr.finish(orr.block_reduce(acc.reshape(blocks, orr.KT, 6), MASKED_OPS), MASKED_CLEAR, MASKED_OPS)
    else:
        tot = MASKED_CLEAR
    out[0], out[7] = tot[0], tot[5]
    if tot[0] > 0:
        out[1:5] = tot[1:5]
        counted = v[on & fin]
        for i, q in enumerate(percentiles):
            out[5 + i] = np.float64(np.percentile(counted, q))
    return out


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def edt_field(shape, spacing_xyz, seed, roll=None):
    """The squared EDT to the complement of rolled blobs (the set touches the border, windows are clipped on every face): the field of
    radius="voxel".  By edt_ref's line form, which its own tests pin to the brute force."""
    roll = tuple(n // 3 for n in shape) if roll is None else roll
    comp = ~edt_ref.in_set(edt_ref.blobs(shape, seed, roll))
    return edt_ref.edt_sq_lines(comp, spacing_xyz) if comp.any() else np.full(shape, np.inf)


def generic_field(shape, spacing_xyz, seed):
    """A random field from no geometry at all: squared radii up to a few voxels' worth, one voxel in three a non-centre of every
    kind -- NaN, +inf, -inf, negative, zero."""
    rng = np.random.default_rng([seed, *shape])
    s = float(max(spacing_xyz))
    f = (rng.uniform(0.2, 3.2, size=shape) * s) ** 2
    kind = rng.integers(0, 15, size=shape)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -1.5, 0.0)):
        f[kind == k] = bad
    return f


def slab(shape, t, z0=2):
    """A float32 map: a slab of t voxels along z, through the whole of y and x."""
    v = np.zeros(shape, np.float32)
    v[z0:z0 + t] = 1.0
    return v


def ball(shape, radius):
    """A float32 map: the voxels within ``radius`` voxels of the centre of the volume."""
    z, y, x = np.meshgrid(*(np.arange(n) - (n - 1) / 2.0 for n in shape), indexing="ij")
    return ((x * x + y * y + z * z) <= radius * radius).astype(np.float32)
