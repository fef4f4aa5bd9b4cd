"""numpy restatement of csrc/thickness_image.hip (include/oai_hip.h, "Thickness image"): the same fp64 operations in the same order,
so owner and corners must come out equal and the weights within two divisions' rounding.  Plain loops over faces; each face is
tested against a box of pixel centres that only has to be conservative (here: one pixel of margin, found by comparison)."""
import numpy as np


def grid(uv, image_shape):
    """(lo[2], step[2]) of the raster over the finite points: one step per axis."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    fin = uv[np.isfinite(uv).all(axis=1)]
    H, W = image_shape
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    return lo, np.array([(hi[0] - lo[0]) / W, (hi[1] - lo[1]) / H])


def centres(lo, step, image_shape):
    H, W = image_shape
    return lo[0] + (np.arange(W, dtype=np.float64) + 0.5) * step[0], lo[1] + (np.arange(H, dtype=np.float64) + 0.5) * step[1]


def _tri(uv, face, n_pts):
    a, b, c = (int(x) for x in face)
    if min(a, b, c) < 0 or max(a, b, c) >= n_pts:
        return None
    A, B, C = uv[a], uv[b], uv[c]
    if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()):
        return None
    area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    if not np.isfinite(area) or area == 0.0:
        return None
    return A, B, C, area < 0.0


def edge_functions(A, B, C, flip, pu, pv):
    e0 = (C[0] - B[0]) * (pv - B[1]) - (C[1] - B[1]) * (pu - B[0])
    e1 = (A[0] - C[0]) * (pv - C[1]) - (A[1] - C[1]) * (pu - C[0])
    e2 = (B[0] - A[0]) * (pv - A[1]) - (B[1] - A[1]) * (pu - A[0])
    return (-e0, -e1, -e2) if flip else (e0, e1, e2)


def build(uv, faces, face_skip, lo, step, image_shape, whole_image=False):
    """(owner int32 [H,W], corners int32 [H,W,3], weights float64 [H,W,3]).  ``whole_image``: test every face against every pixel
    (the check that the boxes are conservative)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    faces = np.asarray(faces).reshape(-1, 3)
    H, W = image_shape
    pu, pv = centres(np.asarray(lo, np.float64), np.asarray(step, np.float64), image_shape)
    owner = np.full((H, W), -1, np.int32)
    corners = np.zeros((H, W, 3), np.int32)
    weights = np.zeros((H, W, 3), np.float64)
    with np.errstate(all="ignore"):
        for f in range(len(faces)):
            if face_skip is not None and face_skip[f]:
                continue
            t = _tri(uv, faces[f], len(uv))
            if t is None:
                continue
            A, B, C, flip = t
            if whole_image:
                ii, jj = np.arange(W), np.arange(H)
            else:
                us, vs = (A[0], B[0], C[0]), (A[1], B[1], C[1])
                ii = np.nonzero((pu >= min(us) - step[0]) & (pu <= max(us) + step[0]))[0]
                jj = np.nonzero((pv >= min(vs) - step[1]) & (pv <= max(vs) + step[1]))[0]
            if len(ii) == 0 or len(jj) == 0:
                continue
            PU, PV = np.meshgrid(pu[ii], pv[jj])
            e0, e1, e2 = edge_functions(A, B, C, flip, PU, PV)
            take = (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (owner[np.ix_(jj, ii)] < 0)      # ascending f: the first to cover owns
            if not take.any():
                continue
            s = (e0 + e1) + e2
            J, I = jj[np.nonzero(take)[0]], ii[np.nonzero(take)[1]]
            owner[J, I] = f
            corners[J, I] = faces[f]
            weights[J, I] = np.stack([e0[take] / s[take], e1[take] / s[take], e2[take] / s[take]], axis=1)
    return owner, corners, weights


def apply(owner, corners, weights, values):
    """float32 [H,W] for values [n], [K,H,W] for values [K,n]; NaN where no face owns the pixel."""
    v = np.asarray(values, np.float32)
    single = v.ndim == 1
    t = np.atleast_2d(v).astype(np.float64)
    a, b, c = corners[..., 0], corners[..., 1], corners[..., 2]
    with np.errstate(all="ignore"):
        img = ((weights[..., 0] * t[:, a] + weights[..., 1] * t[:, b]) + weights[..., 2] * t[:, c]).astype(np.float32)
    img[:, owner < 0] = np.float32(np.nan)
    return img[0] if single else img


def warped_grid(n=60, seed=0, amp=0.25):
    """An n x n vertex grid over [0,1]^2, interior vertices jittered by < amp of a cell (no fold-overs), two triangles per cell."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, n)
    v, u = np.meshgrid(g, g, indexing="ij")
    uv = np.stack([u, v], axis=-1)
    uv[1:-1, 1:-1] += rng.uniform(-amp, amp, size=(n - 2, n - 2, 2)) / (n - 1)
    uv = uv.reshape(-1, 2) * np.array([3.0, 40.0]) + np.array([-1.0, 7.0])           # axes of unlike units, as angle against mm
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return uv, faces


def soup(seed=1, n_pts=400, n_faces=900):
    """Random triangles with overlaps, both orientations, repeated faces, degenerate faces and one non-finite point."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1, size=(n_pts, 2)) * np.array([6.0, 90.0])
    near = rng.integers(0, n_pts, n_faces)
    d = np.abs(uv[:, None, 0] - uv[None, near, 0]) / 6.0 + np.abs(uv[:, None, 1] - uv[None, near, 1]) / 90.0
    pick = np.argsort(d, axis=0)[:12]                                                # each face from points close to a seed point
    faces = np.stack([pick[rng.integers(0, 12, n_faces), np.arange(n_faces)] for _ in range(3)], axis=1)
    faces[::37, 1] = faces[::37, 0]                                                  # degenerate: a repeated corner
    faces[5::41] = faces[4::41][:len(faces[5::41])]                                  # the same face twice
    uv[7] = np.nan
    return uv, faces.astype(np.int32)
