"""Small deterministic meshes for the edges of the device inner / outer split (csrc/mesh_split.hip), each from a seed and an exact
face count (not collected).  tests/test_mesh_split_edges_cpu.py shows with the restatement (tests/mesh_split_ref.py) that the list
reaches every path it is meant to reach; tests/test_mesh_split_edges_gpu.py runs the list on the device.

Two families, both a pair of wavy parallel sheets with opposite windings (an inner and an outer surface), cut into triangles:
  sheets  flat along x and z, the normals along -+ y; x on a lattice of halves, as a voxel mesh has it.  The FC family.
  arch    the same pair bent round the z axis through ARCH_SPAN radians, so that the normals sweep most of a circle and the two
          clusters of the TC fit are not the two sheets.  The TC family: its Lloyd loop runs longer and also stops on tol.
The faces of a pool a little larger than asked for are shuffled and cut to the face count; the pool's vertices all stay, so every
mesh also has vertices that no face uses."""
from dataclasses import dataclass

import numpy as np

SIZES = (2, 3, 63, 65, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097)     # around a wave, the workgroup and the cumulative-sum tile
FC_TOTALS = SIZES[2:]                                                     # three slabs of at least 2 faces need more than 3 faces
# FC meshes with chosen sizes of slab 0 and slab 1: every size of SIZES as one nine-column fit
FC_SLAB_COUNTS = ((2, 3, 40), (63, 65, 50), (511, 513, 300), (2047, 2048, 700), (2049, 4095, 900), (4096, 4097, 1100))
SUM_SIZES = (15, 16, 17, 4095, 4096, 4097, 8193)                          # col_sum_seq_kernel: its unroll by 16 and its 4096-row tile
ARCH_SPAN = 4.4
BIG_FACES = 65536 + 300                                                   # minmax_kernel strides by 65536


@dataclass
class Case:
    name: str
    mesh_type: str           # "FC" | "TC"
    verts: np.ndarray        # float32 [V, 3]
    faces: np.ndarray        # int32 [F, 3]


def _pool(rng, n_faces, arch):
    """(verts, faces) of the two sheets with at least n_faces faces: 3 k x k quads per sheet, two triangles per quad"""
    k = 1
    while 12 * k * k < n_faces + n_faces // 4 + 8:
        k += 1
    nx, nz = 3 * k, k
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
    amp, fx, fz, px, pz = rng.uniform(0.3, 0.8), rng.uniform(0.3, 0.9), rng.uniform(0.5, 1.3), rng.uniform(0, 6.28), rng.uniform(0, 6.28)
    x = i * 0.5
    z = j * 0.5 + rng.uniform(-0.15, 0.15, i.shape)
    wave = amp * np.sin(fx * x + px) * np.cos(fz * z + pz) + rng.uniform(-0.03, 0.03, i.shape)
    thick = 1.5 + 0.4 * np.sin(0.37 * x + pz) + rng.uniform(-0.03, 0.03, i.shape)
    sheets = []
    for y in (wave, wave + thick):
        if arch:
            theta = (x / x.max() - 0.5) * ARCH_SPAN
            radius = 0.35 * x.max() + y
            sheets.append(np.stack([radius * np.sin(theta), radius * np.cos(theta), z], axis=-1))
        else:
            sheets.append(np.stack([x, y, z], axis=-1))
    verts = np.concatenate([s.reshape(-1, 3) for s in sheets]).astype(np.float32)
    idx = np.arange((nx + 1) * (nz + 1)).reshape(nx + 1, nz + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    lower = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    upper = lower[:, ::-1] + idx.size                                     # the outer sheet: the opposite winding
    return verts, np.concatenate([lower, upper]).astype(np.int32)


def _centroid_x(verts, faces):
    return verts.astype(np.float64)[faces][:, :, 0].sum(axis=1) / 3.0


def cut(seed, n_faces, arch):
    """the family's mesh of exactly n_faces faces"""
    rng = np.random.default_rng(seed)
    verts, faces = _pool(rng, n_faces, arch)
    return verts, np.ascontiguousarray(faces[rng.permutation(len(faces))[:n_faces]])


def fc_slabs(seed, counts, arch=False):
    """An FC mesh whose slab 0 and slab 1 hold exactly counts[0] and counts[1] faces and slab 2 about counts[2]: faces drawn by the
    third of the centroid x range they lie in (1e-3 of the range clear of the seams), with the faces of least and greatest x kept
    so that the range is the pool's.  The face of greatest x is the last face and alone there: a half-open slab 2 may leave it out."""
    rng = np.random.default_rng(seed)
    verts, faces = _pool(rng, 2 * sum(counts), arch)
    cx = _centroid_x(verts, faces)
    lo, hi = int(np.argmin(cx)), int(np.argmax(cx))
    t = (cx - cx[lo]) / (cx[hi] - cx[lo]) * 3.0
    pick = [lo]
    for s, m in enumerate(counts):
        inside = np.flatnonzero((t > s + 1e-3) & (t < s + 1 - 1e-3))
        pick.extend(rng.permutation(inside)[:m - (s == 0)])
    pick = np.array(pick)[rng.permutation(len(pick))]
    return verts, np.ascontiguousarray(faces[np.append(pick, hi)])


def big(seed):
    """BIG_FACES faces on more than 65536 vertices.  The last six faces, on eighteen vertices of their own at the end, lie just
    outside the sheets, one beyond each end of each axis: every least and greatest centroid and vertex coordinate has an index of
    65536 or more, where only the second pass of a 65536-wide grid-stride loop looks."""
    rng = np.random.default_rng(seed)
    verts, faces = _pool(rng, 140000, False)                              # 363 x 121 quads per sheet: 88816 vertices
    faces = faces[rng.permutation(len(faces))[:BIG_FACES - 6]]
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    mid = (lo + hi) / 2
    extra_v, extra_f = [], []
    for axis in range(3):
        for end, sign in ((lo, -1.0), (hi, 1.0)):
            p = mid.copy()
            p[axis] = end[axis] + sign * 0.25
            u, w = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3], w[(axis + 2) % 3] = 0.2, 0.2
            tip = np.zeros(3)
            tip[axis] = sign * 0.125                                      # the face's own extreme vertex
            base = len(verts) + len(extra_v)
            extra_v += [p + tip, p + u, p + w]
            extra_f.append([base, base + 1, base + 2])
    verts = np.concatenate([verts, np.array(extra_v, np.float32)])
    return verts, np.ascontiguousarray(np.concatenate([faces, np.array(extra_f, np.int32)]))


def degenerate(seed, arch):
    """200 faces of the family, a face (v, v, w) of zero area, whose normal is 0, and a sliver on three vertices that are collinear up to
    their rounding to float32, whose normal is whatever that rounding left"""
    verts, faces = cut(seed, 200, arch)
    a, b = verts[faces[0, 0]], verts[faces[0, 1]]
    n = len(verts)
    verts = np.concatenate([verts, np.array([a, a + (b - a) * np.float32(0.5), a + (b - a) * np.float32(2)], np.float32)])
    extra = np.array([[faces[1, 0], faces[1, 0], faces[1, 2]], [n, n + 1, n + 2]], np.int32)
    return verts, np.ascontiguousarray(np.concatenate([faces[:120], extra, faces[120:]]))


def bad_indices(seed):
    """a mesh of 300 faces, one of which names the vertex one past the end and one a negative vertex"""
    verts, faces = cut(seed, 300, False)
    faces = faces.copy()
    faces[7, 1] = len(verts)
    faces[290, 2] = -1
    return verts, faces


# The seeds: any for which the restatement meets the margins tests/test_mesh_split_edges_cpu.py asks for.  Three samples need a
# chosen one: where the two nearest of them are the two candidates of a k-means++ trial, both trials have the same potential in
# exact arithmetic, and rounding alone picks the second centre.
_SEEDS = {"arch-tc-3": 108, "sheets-fc-slabs-2-3": 100}


def cases():
    """every mesh that goes through the k-means of both the restatement and the device"""
    out = []

    def add(name, mesh_type, build, seed, *args):
        out.append(Case(name, mesh_type, *build(_SEEDS.get(name, seed), *args)))
    for n in SIZES:
        add(f"arch-tc-{n}", "TC", cut, 100 + n, n, True)
    for n in FC_TOTALS:
        add(f"sheets-fc-{n}", "FC", cut, 200 + n, n, False)
    for k, counts in enumerate(FC_SLAB_COUNTS):
        add(f"sheets-fc-slabs-{counts[0]}-{counts[1]}", "FC", fc_slabs, 300 + k, counts)
    add("arch-fc-513", "FC", cut, 400, 513, True)
    add("sheets-tc-2049", "TC", cut, 401, 2049, False)
    for arch in (False, True):
        for mesh_type in ("FC", "TC"):
            add(f"degenerate-{'arch' if arch else 'sheets'}-{mesh_type.lower()}", mesh_type, degenerate, 410 + arch, arch)
    return out


def big_case(mesh_type):
    return Case(f"big-{mesh_type.lower()}", mesh_type, *big(500))


# hand-picked draws, one init per slab: (first centre, (u0, u1)) from the slab's size
HAND_DRAWS = {
    "clip": lambda n: (0, (1 - 2.0 ** -53, 1 - 2.0 ** -53)),      # r = pot less half an ulp: the search ends at n - 1 or past the end
    "zero": lambda n: (n // 2, (0.0, 0.618)),                     # a draw of exactly 0: the candidate is sample 0
    "last": lambda n: (n - 1, (0.3, 0.7)),                        # the first centre is the last sample
    "empty": lambda n: (0, (0.0, 0.0)),                           # both candidates are the first centre: the second cluster is empty
}
HAND_DRAW_MESHES = ("arch-tc-65", "arch-tc-513", "arch-tc-2048", "sheets-fc-513", "sheets-fc-slabs-2047-2048")


def hand_draws(kind, slab_sizes):
    """slab_draws for mesh_split_ref.split_sides_draws(n_init=1): ([first], [[u0, u1]]) per slab"""
    return [([HAND_DRAWS[kind](int(n))[0]], [HAND_DRAWS[kind](int(n))[1]]) for n in slab_sizes]
