"""numpy restatement of the cuberille contract (include/oai_hip.h, csrc/cuberille.hip), literal and in fp64 with the kernels'
operation order, so that the device result can be compared bit for bit: face order, first-use vertex numbering, winding, and the
projection loop (every vertex walked one step at a time with the same IEEE operations; numpy never contracts)."""
import numpy as np

# neighbour j = -z -y -x +x +y +z: (axis in xyz, + side)
NEIGHBOURS = ((2, False), (1, False), (0, False), (0, True), (1, True), (2, True))
_PLUS = ((0, 0), (1, 0), (1, 1), (0, 1))
_MINUS = ((0, 0), (0, 1), (1, 1), (1, 0))


def geometry(spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
    """(origin, spacing, direction, M) as float64 arrays; M = inv(direction diag(spacing)), the matrix the device is given."""
    s = np.asarray(spacing, np.float64).reshape(3)
    o = np.asarray(origin, np.float64).reshape(3)
    d = np.eye(3) if direction is None else np.asarray(direction, np.float64).reshape(3, 3)
    return o, s, d, np.linalg.inv(d @ np.diag(s))


def faces_and_lattice(vol, iso=0.5):
    """(quads int64 [m,4] of vertex ids, lattice xyz int64 [n,3] of each vertex, the (voxel, neighbour) pairs [m,2])."""
    vol = np.asarray(vol, np.float32)
    D, H, W = vol.shape
    inside = vol >= np.float32(iso)
    pad = np.pad(inside, 1, constant_values=False)
    outs = []
    for a, plus in NEIGHBOURS:
        sl = [slice(1, D + 1), slice(1, H + 1), slice(1, W + 1)]
        zyx = 2 - a
        sl[zyx] = slice(2, D + 2 if zyx == 0 else (H + 2 if zyx == 1 else W + 2)) if plus else slice(0, (D, H, W)[zyx])
        outs.append(inside & ~pad[tuple(sl)])
    pairs = np.argwhere(np.stack(outs, axis=-1).reshape(-1, 6))          # C order: voxel-major, neighbour-minor
    vox, j = pairs[:, 0], pairs[:, 1]
    z, y, x = vox // (H * W), (vox // W) % H, vox % W
    base = np.stack([x, y, z], axis=1)
    corners = np.zeros((len(vox), 4, 3), np.int64)
    for jj, (a, plus) in enumerate(NEIGHBOURS):
        sel = j == jj
        b, c = (a + 1) % 3, (a + 2) % 3
        for q, (ob, oc) in enumerate(_PLUS if plus else _MINUS):
            p = base[sel].copy()
            p[:, a] += 1 if plus else 0
            p[:, b] += ob
            p[:, c] += oc
            corners[sel, q] = p
    key = (corners[..., 2] * (H + 1) + corners[..., 1]) * (W + 1) + corners[..., 0]
    flat = key.reshape(-1)
    uniq, first = np.unique(flat, return_index=True)
    order = uniq[np.argsort(first, kind="stable")]
    remap = np.full((D + 1) * (H + 1) * (W + 1), -1, np.int64)
    remap[order] = np.arange(len(order))
    lat = np.stack([order % (W + 1), (order // (W + 1)) % (H + 1), order // ((W + 1) * (H + 1))], axis=1)
    return remap[key], lat, pairs


def physical(lat, geo):
    o, s, d, _ = geo
    u = [s[k] * (lat[:, k].astype(np.float64) - 0.5) for k in range(3)]
    return np.stack([o[r] + ((d[r, 0] * u[0] + d[r, 1] * u[1]) + d[r, 2] * u[2]) for r in range(3)], axis=1)


def _lerp(a, b, t):
    return a + t * (b - a)


def gradient_volume(vol, spacing):
    """Per-voxel index-space gradient (x, y, z components) by central differences with replicated borders, fp64."""
    f = np.asarray(vol, np.float32).astype(np.float64)
    out = []
    for k, ax in ((0, 2), (1, 1), (2, 0)):                       # x is the last array axis
        n = f.shape[ax]
        ip = np.minimum(np.arange(n) + 1, n - 1)
        im = np.maximum(np.arange(n) - 1, 0)
        out.append((np.take(f, ip, axis=ax) - np.take(f, im, axis=ax)) / (2.0 * spacing[k]))
    return out


def sample(vol64, grads, geo, p):
    """(value, physical gradient [n,3]) at physical points p [n,3]."""
    o, _, d, M = geo
    D, H, W = vol64.shape
    e = [p[:, r] - o[r] for r in range(3)]
    c = [(M[k, 0] * e[0] + M[k, 1] * e[1]) + M[k, 2] * e[2] for k in range(3)]
    i0, i1, t = [], [], []
    for k, n in enumerate((W, H, D)):
        hi = float(n - 1)
        cc = np.where(c[k] < 0.0, 0.0, np.where(c[k] > hi, hi, c[k]))
        a = np.floor(cc).astype(np.int64)
        a = np.maximum(np.minimum(a, n - 2), 0)
        i0.append(a)
        i1.append(np.minimum(a + 1, n - 1))
        t.append(cc - a.astype(np.float64))

    def tri(f):
        g = [f[(i1[2] if cz else i0[2]), (i1[1] if cy else i0[1]), (i1[0] if cx else i0[0])]
             for cz in (0, 1) for cy in (0, 1) for cx in (0, 1)]            # corner bit 0: x, bit 1: y, bit 2: z
        a, b, cc, dd = _lerp(g[0], g[1], t[0]), _lerp(g[2], g[3], t[0]), _lerp(g[4], g[5], t[0]), _lerp(g[6], g[7], t[0])
        return _lerp(_lerp(a, b, t[1]), _lerp(cc, dd, t[1]), t[2])

    val = tri(vol64)
    gi = [tri(g) for g in grads]
    grad = np.stack([(d[r, 0] * gi[0] + d[r, 1] * gi[1]) + d[r, 2] * gi[2] for r in range(3)], axis=1)
    return val, grad


def project(vol, p0, geo, iso=0.5, threshold=0.05, step_length=-1.0, relaxation=0.95, max_steps=50, move_after_converged=True):
    """The projection loop of the contract for every vertex: (p float64 [n,3], k int32 [n])."""
    vol64 = np.asarray(vol, np.float32).astype(np.float64)
    grads = gradient_volume(vol, geo[1])
    iso64 = np.float64(np.float32(iso))
    L = 0.25 * float(np.max(geo[1])) if step_length < 0 else float(step_length)
    p = np.array(p0, np.float64, copy=True)
    n = len(p)
    step = np.full(n, L)
    k = np.zeros(n, np.int32)
    active = np.arange(n)
    while len(active):
        val, g = sample(vol64, grads, geo, p[active])
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        m = val - iso64
        done = np.abs(m) <= threshold
        stop = (ln == 0.0) | (done & (not move_after_converged))
        mv = ~stop
        idx = active[mv]
        s = np.where(m[mv] < 0.0, step[idx], -step[idx])
        p[idx] = p[idx] + s[:, None] * (g[mv] / ln[mv][:, None])
        k[idx] += 1
        fin = done[mv] | (k[idx] > max_steps)
        step[idx] = step[idx] * relaxation
        active = idx[~fin]
    return p, k


def cuberille(vol, iso=0.5, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None, triangles=True, project_vertices=True,
              threshold=0.05, step_length=-1.0, relaxation=0.95, max_steps=50, move_after_converged=True):
    """dict: verts (float32), verts64 (fp64 before the float32 store), faces (int32 [2m,3] or [m,4]), steps (int32), quads, lattice."""
    geo = geometry(spacing, origin, direction)
    quads, lat, _ = faces_and_lattice(vol, iso)
    p = physical(lat, geo)
    k = np.zeros(len(p), np.int32)
    if project_vertices and len(p):
        p, k = project(vol, p, geo, iso, threshold, step_length, relaxation, max_steps, move_after_converged)
    flip = np.linalg.det(geo[2]) < 0
    q = quads[:, [0, 3, 2, 1]] if flip else quads
    if triangles:
        t = np.empty((2 * len(q), 3), np.int64)
        if flip:
            t[0::2] = quads[:, [0, 2, 1]]
            t[1::2] = quads[:, [0, 3, 2]]
        else:
            t[0::2] = quads[:, [0, 1, 2]]
            t[1::2] = quads[:, [0, 2, 3]]
        faces = t
    else:
        faces = q
    return dict(verts=p.astype(np.float32), verts64=p, faces=faces.astype(np.int32), steps=k, quads=quads, lattice=lat)


def signed_volume6(verts, tris, center=True):
    """6 x the enclosed signed volume, fp64 (about the vertices' mean when ``center``; without it, exact on half-integer vertices)."""
    v = np.asarray(verts, np.float64)
    if center:
        v = v - v.mean(axis=0)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.sum(a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])
                        + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])))


def ellipsoid_case(shape=(36, 40, 36), spacing=(0.6, 0.5, 0.7), axes=None, slope=2.0):
    """An analytic ellipsoid map: value 0.5 - slope * R (q - 1), q = |((p - c) / axes)|, R = the mean semi-axis (the slope is about
    ``slope`` per mm across the 0.5 surface q = 1).  dict(vol, spacing, centre, axes, volume, distance(p) = first-order distance of
    physical points p to the surface)."""
    D, H, W = shape
    sp = np.asarray(spacing, np.float64)
    ext = np.array([W, H, D]) * sp
    c0 = ext / 2 + np.array([0.13, -0.21, 0.07])
    ax = np.asarray(axes, np.float64) if axes is not None else ext * np.array([0.36, 0.3, 0.4])
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float64)
    q = np.sqrt(((x * sp[0] - c0[0]) / ax[0]) ** 2 + ((y * sp[1] - c0[1]) / ax[1]) ** 2 + ((z * sp[2] - c0[2]) / ax[2]) ** 2)
    vol = (0.5 - slope * ax.mean() * (q - 1.0)).astype(np.float32)

    def distance(p):
        u = (np.asarray(p, np.float64) - c0) / ax
        qq = np.sqrt((u ** 2).sum(axis=1))
        g = np.linalg.norm(u / ax / qq[:, None], axis=1)
        return np.abs(qq - 1.0) / g

    return dict(vol=vol, spacing=tuple(sp), centre=c0, axes=ax, volume=4.0 / 3.0 * np.pi * np.prod(ax), distance=distance)


def last_step(steps, L, relaxation=0.95):
    """The length of each vertex's last move (0 for a vertex that never moved)."""
    k = np.asarray(steps, np.int64)
    return np.where(k > 0, L * relaxation ** np.maximum(k - 1, 0).astype(np.float64), 0.0)
