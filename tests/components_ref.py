"""numpy restatement of csrc/components.hip (include/oai_hip.h, "Segmentation-shape QC"), written from the header text: a union-find
over the voxels of the labelled set with the smallest linear index as representative (hook the larger root under the smaller, jump
the parents, until no joined pair has two roots), the raster-order numbering as a scan of the root flags, and the twelve summary
slots; with the shapes and the seeded and fixed layouts that the CPU and GPU tests share.  Not collected as a test."""
import numpy as np

CONNECTIVITIES = (6, 18, 26)
DENSITIES = (0.02, 0.1, 0.31, 0.6, 1.0, 0.0)       # 0.31 and 0.1: the site-percolation thresholds of 6 and 26 connectivity
SHAPES_CPU = [(1, 1, 1), (1, 5, 7), (5, 6, 7), (9, 14, 17), (3, 4, 70)]
BRICK = (4, 4, 64)                                 # csrc/components.hip: kBZ, kBY, kBX
# one voxel; flat; odd tails; x longer than a block's threads; long y; long z; one voxel past a brick on every axis; many bricks
SHAPES_GPU = [(1, 1, 1), (1, 5, 7), (9, 14, 17), (3, 4, 300), (5, 300, 4), (260, 3, 2), (17, 33, 65), (40, 96, 96)]
SHAPES_FIXED = [(17, 33, 65), (9, 14, 17)]

# the neighbours that precede a voxel in raster order (dz, dy, dx): faces, edges, corners -- the other half is the mirror image
BACK = [(0, 0, -1), (0, -1, 0), (-1, 0, 0),
        (0, -1, -1), (0, -1, 1), (-1, 0, -1), (-1, 0, 1), (-1, -1, 0), (-1, 1, 0),
        (-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1)]


def dual(connectivity):
    """The connectivity of the background that goes with a foreground connectivity."""
    return 26 if connectivity == 6 else 6


def the_set(vol, threshold=0.5, complement=False):
    """Membership by the header's rule: a float32 map -- finite and > threshold; any other dtype -- != 0."""
    vol = np.asarray(vol)
    if vol.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            s = np.isfinite(vol) & (np.nan_to_num(vol, nan=0.0, posinf=0.0, neginf=0.0) > np.float32(threshold))
    else:
        s = vol != 0
    return ~s if complement else s


def _joined_pairs(s, connectivity):
    """(a, b) flat indices of every pair of voxels of the set that the connectivity joins, each pair once."""
    D, H, W = s.shape
    idx = np.arange(s.size, dtype=np.int64).reshape(s.shape)
    a, b = [], []
    for dz, dy, dx in BACK[:{6: 3, 18: 9, 26: 13}[connectivity]]:
        z0, z1 = max(0, -dz), D - max(0, dz)
        y0, y1 = max(0, -dy), H - max(0, dy)
        x0, x1 = max(0, -dx), W - max(0, dx)
        if z0 >= z1 or y0 >= y1 or x0 >= x1:
            continue
        p = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        q = (slice(z0 + dz, z1 + dz), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
        both = s[p] & s[q]
        a.append(idx[p][both])
        b.append(idx[q][both])
    return (np.concatenate(a), np.concatenate(b)) if a else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def roots_ref(s, connectivity):
    """int64 [D,H,W]: per voxel of the set the smallest linear index of its component, -1 off the set."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(connectivity)
    parent = np.arange(s.size, dtype=np.int64)
    a, b = _joined_pairs(s, connectivity)
    while a.size:
        ra, rb = parent[a], parent[b]                  # roots: the parents are fully jumped at this point
        differ = ra != rb
        if not differ.any():
            break
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))      # hook: a link only ever moves to a smaller index
        while True:                                    # jump
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return np.where(s.ravel(), parent, -1).reshape(s.shape)


def label_ref(vol, threshold=0.5, connectivity=26, complement=False, min_voxels=0):
    """(labels int32, size map int32, summary int64 [12]) of oai_label_components."""
    vol = np.asarray(vol)
    s = the_set(vol, threshold, complement)
    D, H, W = s.shape
    root = roots_ref(s, connectivity).ravel()
    flat = np.arange(s.size, dtype=np.int64)
    is_root = root == flat
    rank = np.cumsum(is_root) - is_root                # exclusive scan of the root flags: raster order of the first voxels
    labels = np.where(root >= 0, rank[np.maximum(root, 0)] + 1, 0).astype(np.int32)
    K = int(is_root.sum())
    sizes = np.bincount(labels, minlength=K + 1)[1:].astype(np.int64)      # by label
    size_map = np.where(labels > 0, sizes[np.maximum(labels, 1) - 1] if K else 0, 0).astype(np.int32)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    on_border = ((z == 0) | (z == D - 1) | (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).ravel()
    touches = np.zeros(K + 1, bool)
    touches[labels[on_border & (labels > 0)]] = True
    touches = touches[1:]
    order = np.sort(sizes)[::-1]
    small = sizes < min_voxels
    summary = np.array([s.size, int(s.sum()), K,
                        int(order[0]) if K else 0, int(np.argmax(sizes)) + 1 if K else 0,      # argmax: the first, i.e. the smallest label
                        int(order[1]) if K > 1 else 0,
                        int(small.sum()), int(sizes[small].sum()), int(touches.sum()), int(sizes[touches].sum()),
                        int((~np.isfinite(vol)).sum()) if vol.dtype == np.float32 else 0, 0], np.int64)
    return labels.reshape(s.shape), size_map.reshape(s.shape), summary


def shape_record(fg, bg, n_over_lo, n_over_hi, connectivity, min_voxels, voxel_mm3=None):
    """The figures of qc.SegmentationShape from the summary of the set (``fg``), the summary of its complement under the dual
    connectivity (``bg``) and the two counts |p > band[0]|, |p > band[1]|, as a dict."""
    voxels, K, largest = int(fg[1]), int(fg[2]), int(fg[3])
    return dict(voxels=voxels, mm3=None if voxel_mm3 is None else voxels * float(voxel_mm3), components=K, largest_voxels=largest,
                largest_fraction=largest / voxels if voxels else float("nan"), islands=max(K - 1, 0), island_voxels=voxels - largest,
                small_components=int(fg[6]), small_voxels=int(fg[7]), border_components=int(fg[8]),
                cavities=int(bg[2] - bg[8]), cavity_voxels=int(bg[1] - bg[9]), uncertain_voxels=int(n_over_lo) - int(n_over_hi),
                nonfinite=int(fg[10]), connectivity=int(connectivity), min_voxels=int(min_voxels))


# ---- seeded and fixed layouts ------------------------------------------------------------------------------------------------------------
def random_mask(shape, density, seed=7):
    """uint8: each voxel in the set with probability ``density`` (1.0: all, 0.0: none)."""
    return (np.random.default_rng(seed).uniform(size=shape) < density).astype(np.uint8)


def as_map(mask, seed=3):
    """A float32 map whose set > 0.5 is ``mask``: values in (0.5, 1] on it and in [0, 0.5] off it (0.5 itself is off the set)."""
    u = np.random.default_rng(seed).uniform(size=mask.shape).astype(np.float32) * np.float32(0.5)
    return np.where(np.asarray(mask) != 0, np.float32(1.0) - u * np.float32(0.999), u).astype(np.float32)


def serpentine(shape):
    """One voxel-wide path: every second row of every second slice, neighbouring rows joined alternately at the two x ends, neighbouring
    slices joined alternately at the path's end and at its start.  One component under every connectivity; its length is of the order
    of the volume."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, H, 2))
    m[::2, ::2, :] = 1
    for k, y in enumerate(rows[:-1]):
        m[::2, y + 1, W - 1 if k % 2 == 0 else 0] = 1
    end = (rows[-1], 0 if len(rows) % 2 == 0 else W - 1)           # where the path that starts at (0, 0) leaves the slice
    for k, z in enumerate(range(0, D - 2, 2)):
        y, x = end if k % 2 == 0 else (0, 0)
        m[z + 1, y, x] = 1
    return m


def comb(shape):
    """Teeth along x in every second row and slice, joined only by the plane x = W - 1."""
    m = np.zeros(shape, np.uint8)
    m[::2, ::2, :] = 1
    m[:, :, -1] = 1
    return m


def checkerboard(shape):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def touching_pairs(shape):
    """[(name, kind, a, b)]: two voxels that touch by an ``edge`` only or by a ``corner`` only, placed inside a brick and across a
    brick face, edge and corner (as far as the shape has more than one brick along the axes involved).  Components under 6 / 18 / 26:
    edge 2 / 1 / 1, corner 2 / 2 / 1."""
    D, H, W = shape
    bz, by, bx = BRICK
    out = [("edge inside", "edge", (1, 1, 1), (1, 2, 2)), ("corner inside", "corner", (1, 1, 1), (2, 2, 2)),
           ("edge across a y face", "edge", (1, by - 1, 1), (1, by, 2)), ("edge across a z face", "edge", (bz - 1, 1, 1), (bz, 1, 2)),
           ("edge across a zy edge", "edge", (bz - 1, by - 1, 1), (bz, by, 1)), ("edge across a zy edge, other diagonal", "edge", (bz - 1, by, 1), (bz, by - 1, 1)),
           ("corner across a z face", "corner", (bz - 1, 1, 1), (bz, 2, 2)), ("corner across a zy edge", "corner", (bz - 1, by - 1, 1), (bz, by, 2)),
           ("corner across a zy edge, other diagonals", "corner", (bz - 1, by, 2), (bz, by - 1, 1))]
    if W > bx:
        out += [("edge across an x face", "edge", (1, 1, bx - 1), (1, 2, bx)), ("edge across a yx edge", "edge", (1, by - 1, bx - 1), (1, by, bx)),
                ("edge across a zx edge, other diagonal", "edge", (bz - 1, 1, bx), (bz, 1, bx - 1)),
                ("corner across an x face", "corner", (1, 1, bx - 1), (2, 2, bx)), ("corner across a yx edge", "corner", (1, by - 1, bx - 1), (2, by, bx)),
                ("corner across a brick corner", "corner", (bz - 1, by - 1, bx - 1), (bz, by, bx)),
                ("corner across a brick corner, other diagonals", "corner", (bz - 1, by, bx - 1), (bz, by - 1, bx))]
    for name, kind, a, b in out:
        d = sorted(abs(p - q) for p, q in zip(a, b))
        assert d == ([0, 1, 1] if kind == "edge" else [1, 1, 1]) and all(0 <= v < n for p in (a, b) for v, n in zip(p, shape)), name
    return out


def pair_mask(shape, a, b):
    m = np.zeros(shape, np.uint8)
    m[a], m[b] = 1, 1
    return m


PAIR_COMPONENTS = {"edge": {6: 2, 18: 1, 26: 1}, "corner": {6: 2, 18: 2, 26: 1}}


def hollow_box(shape, pinhole=False):
    """A closed one-voxel shell two voxels inside the volume: one cavity.  ``pinhole``: the shell's first corner voxel removed -- the
    cavity then touches the outside through that voxel by a corner only, so it is closed for a 6-connected background (foreground 18
    or 26) and open for a 26-connected one (foreground 6)."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    m[2:D - 2, 2:H - 2, 2:W - 2] = 1
    m[3:D - 3, 3:H - 3, 3:W - 3] = 0
    assert D >= 7 and H >= 7 and W >= 7
    if pinhole:
        m[2, 2, 2] = 0
    return m


def last_voxel(shape):
    """A few components, the last of which consists of the last voxel of the volume alone."""
    m = np.zeros(shape, np.uint8)
    m[0, 0, 0] = m[shape[0] // 2, shape[1] // 2, shape[2] // 2] = m[-1, -1, -1] = 1
    return m


def planted(shape=(24, 40, 48), seed=5):
    """The blobs of edt_ref with one cavity and two islands planted: a float32 map.  The cavity is one voxel at the deepest point of
    the largest blob (its six face neighbours are in the set); each island is one voxel with nothing of the set within its 26
    neighbours."""
    import edt_ref as er
    v = er.blobs(shape, seed=seed, roll=(2, 5, 3))
    labels, _, summary = label_ref(v)
    inside = _depth(labels == summary[4], 2)
    z, y, x = np.unravel_index(int(np.argmax(inside)), shape)
    assert inside[z, y, x] == 2
    v[z, y, x] = 0.0
    free = np.argwhere(_depth(~the_set(v), 4) == 4)     # nothing of the set within a city-block distance of 3: the 26 neighbours are free
    assert len(free) >= 2 and np.abs(free[0] - free[-1]).max() > 2
    v[tuple(free[0])] = v[tuple(free[-1])] = 0.9
    return v


def _depth(s, cap):
    """Per voxel of ``s`` the number of 6-neighbour erosions it survives, plus one, up to ``cap`` (0 off ``s``); outside the volume
    counts as off."""
    depth = np.zeros(s.shape, np.int64)
    cur = s.copy()
    for _ in range(cap):
        depth += cur
        p = np.pad(cur, 1, constant_values=False)
        cur = (cur & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return depth
