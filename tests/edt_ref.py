"""numpy restatement of csrc/edt.hip (include/oai_hip.h, "Surface-distance QC"): the brute-force Euclidean distance transform on the
canonical expression, its exhaustive separable form, the 6-neighbour surface and the surface-distance figures, with the seeded inputs
the CPU and GPU tests share.  Not collected as a test."""
import numpy as np

SHAPES_SMALL = [(9, 14, 17), (12, 20, 24), (7, 33, 5), (10, 12, 70)]      # odd tails; general; short x, long y; x > 64 lanes
SPACINGS = [(1.0, 1.0, 1.0), (0.36458333, 0.36458333, 0.7), (0.3, 0.7, 1.1)]      # (x, y, z): isotropic, the OAI DESS spacing, anisotropic


def _terms(n, s):
    """fl(((double)(i - j) * s)^2) for every pair of positions on an axis of n voxels: [n, n]."""
    t = (np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64) * np.float64(s)
    return t * t


def edt_sq_brute(features, spacing_xyz, chunk=512):
    """Per voxel p the minimum over every feature voxel q of (tx*tx + ty*ty) + tz*tz, t = (double)(p - q) * spacing, in fp64: the
    definition, over all pairs.  +inf everywhere without a feature."""
    f = np.asarray(features) != 0
    D, H, W = f.shape
    sx, sy, sz = (np.float64(v) for v in spacing_xyz)
    pz, py, px = (a.reshape(-1, 1) for a in np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"))
    out = np.full(D * H * W, np.inf)
    q = np.argwhere(f)
    for i in range(0, len(q), chunk):
        qz, qy, qx = (q[i:i + chunk, c].reshape(1, -1) for c in range(3))
        tx, ty, tz = (px - qx).astype(np.float64) * sx, (py - qy).astype(np.float64) * sy, (pz - qz).astype(np.float64) * sz
        out = np.minimum(out, ((tx * tx + ty * ty) + tz * tz).min(axis=1))
    return out.reshape(D, H, W)


def edt_sq_lines(features, spacing_xyz):
    """The separable form with every line searched exhaustively: the integer |dx| to the row's nearest feature, then min over y' of
    tx*tx + ty*ty, then min over z' of (that) + tz*tz.  Equal to edt_sq_brute bit for bit, because rounding is monotone."""
    f = np.asarray(features) != 0
    D, H, W = f.shape
    sx, sy, sz = spacing_xyz
    big = 1 << 20
    ax = np.abs(np.arange(W)[:, None] - np.arange(W)[None, :])                                 # [x, x']
    dx = np.where(f[:, :, None, :], ax[None, None], big).min(axis=3)                           # [z, y, x]
    tx = np.where(dx < big, dx, 0).astype(np.float64) * np.float64(sx)
    tx2 = np.where(dx < big, tx * tx, np.inf)
    ty2, tz2 = _terms(H, sy), _terms(D, sz)
    a = np.empty((D, H, W))
    for z in range(D):
        a[z] = (tx2[z][None, :, :] + ty2[:, :, None]).min(axis=1)                              # [y, y', x] -> [y, x]
    out = np.empty((D, H, W))
    for y in range(H):
        out[:, y] = (a[None, :, y, :] + tz2[:, :, None]).min(axis=1)                           # [z, z', x] -> [z, x]
    return out


def in_set(vol, threshold=0.5):
    vol = np.asarray(vol, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(vol) & (np.nan_to_num(vol, nan=0.0, posinf=0.0, neginf=0.0) > np.float32(threshold))


def surface_ref(vol, threshold=0.5, mode=1):
    """oai_mask_surface as uint8: mode 0 the set, 2 its complement, 1 the voxels of the set with a face neighbour outside the set or
    outside the volume."""
    s = in_set(vol, threshold)
    if mode == 0:
        return s.astype(np.uint8)
    if mode == 2:
        return (~s).astype(np.uint8)
    p = np.pad(s, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return (s & ~inner).astype(np.uint8)


def surface_distance_ref(surf_a, dist_to_b, surf_b, dist_to_a, percentiles=(95.0,)):
    """The eight figures of oai_surface_distance as a dict, with ``sum_abs`` for the summation bound: counts, fp64 sums of the float32
    distances, maxima, np.percentile of the pooled float32 array."""
    dab = np.asarray(dist_to_b, np.float32)[np.asarray(surf_a) != 0]
    dba = np.asarray(dist_to_a, np.float32)[np.asarray(surf_b) != 0]
    n_a, n_b = int(dab.size), int(dba.size)
    if n_a == 0 or n_b == 0:
        nan = float("nan")
        return dict(n_a=n_a, n_b=n_b, sum_ab=nan, sum_ba=nan, max_ab=nan, max_ba=nan, percentiles=[nan] * len(percentiles), assd=nan,
                    hausdorff=nan)
    pooled = np.concatenate([dab, dba])
    s_ab, s_ba = float(dab.astype(np.float64).sum()), float(dba.astype(np.float64).sum())
    return dict(n_a=n_a, n_b=n_b, sum_ab=s_ab, sum_ba=s_ba, max_ab=float(dab.max()), max_ba=float(dba.max()),
                percentiles=[np.percentile(pooled, q) for q in percentiles], assd=(s_ab + s_ba) / (n_a + n_b),
                hausdorff=float(max(dab.max(), dba.max())))


def edt_dist32(sq):
    """The float32 distance map of fp64 squared distances."""
    return np.sqrt(sq).astype(np.float32)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def sparse_features(shape, density, seed):
    """uint8: each voxel a feature with probability ``density`` (1.0: all, 0.0: none)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=shape) < density).astype(np.uint8)


def blobs(shape, seed, roll=(0, 0, 0), passes=3):
    """A float32 map in [0, 1]: smoothed noise (a periodic 3-tap binomial filter per axis, ``passes`` times -- near Gaussian), stretched
    to the full range and rolled, so that the set > 0.5 is a few blobs that touch the border."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(size=shape)
    for _ in range(passes):
        for ax in range(3):
            v = 0.25 * np.roll(v, 1, ax) + 0.5 * v + 0.25 * np.roll(v, -1, ax)
    v = (v - v.min()) / max(v.max() - v.min(), np.finfo(np.float64).tiny)
    v = np.clip(0.5 + (v - np.median(v)) * 2.0, 0.0, 1.0)
    return np.roll(v, roll, (0, 1, 2)).astype(np.float32)


def box(shape, lo_zyx, size_zyx, value=1.0):
    """A float32 map that is ``value`` in the box and 0 elsewhere."""
    v = np.zeros(shape, np.float32)
    z, y, x = lo_zyx
    d, h, w = size_zyx
    v[z:z + d, y:y + h, x:x + w] = value
    return v
