"""Fixed inputs for the edges of the atlas thickness map (csrc/thickness_map.hip), each from a seed (not collected).
tests/test_thickness_map_edges_cpu.py shows with the restatements (tests/thickness_map_ref.py, tests/morphometry_ref.py) that the cases
reach what they are meant to reach; tests/test_thickness_map_edges_gpu.py runs them on the device.

Every point is stored as float32; the references widen those values to float64 (thickness_map_ref.pairwise_d2).  The map_attributes
cases sit on lattices of halves and carry small integer values, so every squared distance and every fp64 sum is exact in any order:
the device must give the reference's bits on every target, exact ties and footprint-boundary points included."""
from dataclasses import dataclass

import numpy as np

import thickness_map_ref as tref
from morphometry_ref import point_footprint as footprint_ref

SEED = 20250917
N_COMP = 9                                              # three launches of the interpolation kernel: 4 + 4 + 1 components
TILE_N_SRC = (511, 512, 513, 1024, 1025)                # interp_brute_kernel stages 512 source points per step
TILE_N_TGT = (1, 255, 257)                              # ... in blocks of 256 targets
ARC_SIZES = (3, 255, 256, 257, 65535, 65536, 65537, 131073)          # the reductions: 256 threads, a stride of 65 536
PLATEAU_SIZES = ((3, 3), (255, 257), (256, 65537), (70000, 61073))   # (n_left, n_right)
BELOW_50 = np.nextafter(np.float32(50.0), np.float32(0.0))
NAN_BITS = 0x7FC00000


def _values(rng, n):
    return rng.integers(-8, 9, (n, N_COMP)).astype(np.float32)


# ---- map_attributes / point_footprint ----------------------------------------------------------------------------------------------
@dataclass
class MapCase:
    name: str
    src: np.ndarray          # float32 [n_src, 3]
    vals: np.ndarray         # float32 [n_src, N_COMP], small integers
    tgt: np.ndarray          # float32 [n_tgt, 3]
    radius: float = 1.0


def lattice_case() -> MapCase:
    """About 60 % of the integer lattice 12 x 10 x 3 without the block 4 <= x <= 8, 3 <= y <= 7 (the hole forces closest-point
    fallbacks several cells away), 20 of the points once more under other indices, shuffled; targets on the lattice of halves around it."""
    rng = np.random.default_rng(SEED)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(10), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    hole = (g[:, 0] >= 4) & (g[:, 0] <= 8) & (g[:, 1] >= 3) & (g[:, 1] <= 7)
    kept = g[(rng.random(len(g)) < 0.6) & ~hole]
    src = np.concatenate([kept, kept[rng.choice(len(kept), 20, replace=False)]])
    src = src[rng.permutation(len(src))].astype(np.float32)
    tgt = np.stack(np.meshgrid(np.arange(-2, 16, 0.5), np.arange(-2, 14, 0.5), np.arange(-1, 5, 0.5), indexing="ij"), axis=-1)
    return MapCase("lattice", src, _values(rng, len(src)), tgt.reshape(-1, 3).astype(np.float32))


def cross_ring_case() -> MapCase:
    """One target whose two closest sources are both at distance 3 exactly: index 0 at (+3, 0, 0), three cells away, index 1 at
    (-2, -2, -1), two cells away.  The shell walk meets index 1 first and must go on to the next shell.  Nothing else is within 3; the
    far sources only spread the grid."""
    rng = np.random.default_rng(SEED + 1)
    q = np.array([10.5, 10.5, 10.5])
    src = np.array([q + (3, 0, 0), q + (-2, -2, -1), (0.25, 0.25, 0.25), (20, 20, 20), (0.25, 20, 4), (17.5, 3, 19)], np.float32)
    return MapCase("cross_ring", src, _values(rng, len(src)), q[None].astype(np.float32))


def degenerate_cases():
    rng = np.random.default_rng(SEED + 2)
    # every source in the plane z = 5: one cell along z
    src = np.concatenate([rng.integers(0, 41, (300, 2)) * 0.25, np.full((300, 1), 5.0)], axis=1).astype(np.float32)
    tgt = np.concatenate([rng.integers(-4, 49, (500, 2)) * 0.25, rng.integers(6, 15, (500, 1)) * 0.5], axis=1).astype(np.float32)
    planar = MapCase("planar", src, _values(rng, 300), tgt)
    # 600 coincident sources: one cell, a 600-entry cell list, two brute-force tiles; targets on them, inside, on the boundary, outside, far
    src = np.tile(np.array([[3.0, 4.0, 5.0]], np.float32), (600, 1))
    tgt = np.array([(3, 4, 5), (3.5, 4, 5), (4, 4, 5), (3, 3, 5), (3, 4, 6.5), (3.5, 4.5, 5.5), (4, 5, 5), (100, -50, 7), (-1000, 4, 5)], np.float32)
    coincident = MapCase("coincident", src, _values(rng, 600), tgt)
    # 513 sources on a line along x, 1.5 apart: the cell grows to the 512-per-axis limit, 513 x 1 x 1 cells
    src = np.stack([np.arange(513) * 1.5, np.full(513, 2.0), np.full(513, 3.0)], axis=1).astype(np.float32)
    near = np.stack([rng.integers(-8, 3090, 400) * 0.25, 2.0 + rng.integers(-4, 5, 400) * 0.25, 3.0 + rng.integers(-4, 5, 400) * 0.25], axis=1)
    far = np.array([(384.0, 42.0, 3.0), (-30.0, 2.0, 3.0), (800.0, 2.0, -20.0), (0.75, 2.0, 3.0), (767.25, 2.0, 3.0)])
    line = MapCase("line", src[rng.permutation(513)], _values(rng, 513), np.concatenate([near, far]).astype(np.float32))
    return [planar, coincident, line]


def tile_case(n_src: int, n_tgt: int) -> MapCase:
    """The lattice case's sources repeated to n_src points (repeats: coincident points under larger indices, with values of their
    own) and n_tgt of its targets."""
    base = lattice_case()
    rng = np.random.default_rng(SEED + 3)
    pick = rng.permutation(len(base.tgt))[:n_tgt]
    return MapCase(f"tile_{n_src}_{n_tgt}", np.resize(base.src, (n_src, 3)), _values(rng, n_src), base.tgt[pick])


def nan_cases():
    """(some_nan, all_nan): 80 lattice sources of which 6 rows have NaN in x only and 6 have all three NaN (index 0 among them), and
    targets with two NaN rows; then every source NaN."""
    rng = np.random.default_rng(SEED + 4)
    src = rng.integers(0, 13, (80, 3)).astype(np.float32) * np.float32(0.5)
    bad = np.concatenate([[0], 1 + rng.choice(79, 11, replace=False)])
    src[bad[:6]] = np.nan
    src[bad[6:], 0] = np.nan
    tgt = np.stack(np.meshgrid(np.arange(-1, 8, 1.0), np.arange(-1, 8, 1.0), np.arange(-1, 8, 1.5), indexing="ij"), axis=-1).reshape(-1, 3)
    tgt = np.concatenate([tgt, [(np.nan, 2.0, 2.0), (np.nan, np.nan, np.nan)]]).astype(np.float32)
    some = MapCase("some_nan", src, _values(rng, 80), tgt)
    every = MapCase("all_nan", np.full((40, 3), np.nan, np.float32), _values(rng, 40), tgt)
    return some, every


def finite_bounds(case: MapCase, default=((0.0, 0.0, 0.0), (8.0, 8.0, 8.0))):
    """(lo, hi) float64 of the finite source points: the grid a caller passes when some rows are NaN (``default`` when all are)"""
    ok = np.isfinite(case.src).all(axis=1)
    if not ok.any():
        return tuple(np.asarray(d, np.float64) for d in default)
    return case.src[ok].min(axis=0).astype(np.float64), case.src[ok].max(axis=0).astype(np.float64)


def map_reference(case: MapCase):
    """(out float32 [n_tgt, N_COMP], margin, count, nearest_d2, nearest_j) of the restatements.  A NaN source point is never counted
    and never nearest: the restatements see the finite rows, and the indices are mapped back.  A target with no finite distance (a NaN
    target, or no finite source) has NaN values (bits 0x7fc00000), count 0, +inf and -1."""
    ok = np.flatnonzero(np.isfinite(case.src).all(axis=1))
    live = np.isfinite(case.tgt).all(axis=1)
    n = len(case.tgt)
    out = np.full((n, N_COMP), NAN_BITS, np.uint32).view(np.float32)
    margin, count = np.full(n, np.inf), np.zeros(n, np.int32)
    d2, j = np.full(n, np.inf), np.full(n, -1, np.int32)
    if len(ok) and live.any():
        out[live], margin[live] = tref.map_attributes(case.src[ok], case.vals[ok], case.tgt[live], case.radius)
        count[live], d2[live], jj = footprint_ref(case.src[ok], case.tgt[live], case.radius)
        j[live] = ok[jj].astype(np.int32)
    return out, margin, count, d2, j


# ---- circle fit / FC projection ----------------------------------------------------------------------------------------------------
@dataclass
class ArcCase:
    name: str
    verts: np.ndarray        # float32 [n, 3] as an FC mesh stores them: column 0 is the fitted y, column 1 the fitted x
    thickness: np.ndarray    # float32 [n]


def arc_case(name, n, span=2.2, noise=0.4, centre=(61.5, 48.25), seed=0) -> ArcCase:
    """n points of an arc of ``span`` radians about the -x direction (the angles cross +-pi), radius 31 with radial noise, the recipe of
    tests/golden/make_golden_thickness_map.py.  ``centre`` is in the fitted (x, y), after project_thickness swaps the columns."""
    rng = np.random.default_rng(SEED + 100 + seed)
    phi = rng.uniform(np.pi - span / 2, np.pi + span / 2, n)
    rad = 31.0 + noise * rng.normal(0.0, 1.0, n)
    xs, ys = centre[0] + rad * np.cos(phi), centre[1] + rad * np.sin(phi)
    verts = np.stack([ys, xs, rng.uniform(10.0, 90.0, n)], axis=1).astype(np.float32)
    return ArcCase(name, verts, rng.uniform(0.5, 3.5, n).astype(np.float32))


def arc_cases():
    cases = [arc_case(f"arc_{n}", n, seed=k) for k, n in enumerate(ARC_SIZES)]
    cases.append(arc_case("ring_4000", 4000, span=2 * np.pi, seed=20))
    cases.append(arc_case("arc40deg_3000", 3000, span=np.deg2rad(40.0), seed=21))
    cases.append(arc_case("far_centre_3000", 3000, centre=(191.5, 178.25), seed=22))          # patient-space magnitudes
    cases.append(arc_case("exact_3000", 3000, noise=0.0, seed=23))                             # the residual is float32 rounding only
    return cases


def circumcentre(x, y):
    """closed form for three points (float64)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ax, ay, bx, by = x[1] - x[0], y[1] - y[0], x[2] - x[0], y[2] - y[0]
    d = 2.0 * (ax * by - ay * bx)
    ux = (by * (ax * ax + ay * ay) - ay * (bx * bx + by * by)) / d
    uy = (ax * (bx * bx + by * by) - bx * (ax * ax + ay * ay)) / d
    return np.array([x[0] + ux, y[0] + uy]), float(np.hypot(ux, uy))


def half_axis_points(centre=(60.0, 48.0), r=31.0):
    """float32 [n, 3] (x, y, z) on the four half-axes through an integer centre -- (c_x - r, c_y) twice, the second as c_y - 0.0 -- and
    the centre itself"""
    cx, cy = centre
    p = [(cx + r, cy), (cx + 0.5, cy), (cx, cy + r), (cx, cy + 0.25), (cx - r, cy), (cx - r, cy - 0.0), (cx - 0.5, cy), (cx, cy - r),
         (cx, cy - 0.25), (cx, cy)]
    return np.array([(x, y, 10.0 + k) for k, (x, y) in enumerate(p)], np.float32)


# ---- TC plateaus -------------------------------------------------------------------------------------------------------------------
@dataclass
class PlateauCase:
    name: str
    verts: np.ndarray        # float32 [n, 3]
    thickness: np.ndarray    # float32 [n]


def plateau_case(n_left, n_right, n_nan=0, n_split=0, seed=0) -> PlateauCase:
    """Two tilted anisotropic plateaus (standard deviations 9 / 5 / 0.8, the generator's recipe) on either side of z = 50, interleaved
    in point order.  ``n_nan`` further rows have a NaN z (in neither plateau); the ``n_split`` lowest rows of the right plateau are put at
    z == 50.0 exactly and the ``n_split`` highest of the left one at the float32 just below."""
    rng = np.random.default_rng(SEED + 200 + seed)
    scale = np.array([9.0, 5.0, 0.8])

    def plateau(n, centre):
        axes = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        return centre + (rng.normal(size=(n, 3)) * scale) @ axes.T
    left = plateau(n_left, np.array([40.0, 55.0, 30.0])).astype(np.float32)
    right = plateau(n_right, np.array([42.0, 60.0, 72.0])).astype(np.float32)
    left[:, 2] = np.minimum(left[:, 2], np.float32(49.5))
    right[:, 2] = np.maximum(right[:, 2], np.float32(50.0))
    if n_split:                                              # the rows nearest the split, so that the plateaus keep their shape
        left[np.argsort(left[:, 2])[-n_split:], 2] = BELOW_50
        right[np.argsort(right[:, 2])[:n_split], 2] = np.float32(50.0)
    lost = plateau(n_nan, np.array([41.0, 57.0, 50.0])).astype(np.float32)
    lost[:, 2] = np.nan
    v = np.concatenate([left, right, lost])
    v = v[rng.permutation(len(v))]
    name = f"plateaus_{n_left}_{n_right}" + ("_nan" if n_nan else "") + ("_split" if n_split else "")
    return PlateauCase(name, v, rng.uniform(0.5, 3.0, len(v)).astype(np.float32))


def plateau_cases():
    (a, b, c, d) = PLATEAU_SIZES
    return [plateau_case(*a, seed=0), plateau_case(*b, n_nan=50, seed=1), plateau_case(*c, n_split=8, seed=2), plateau_case(*d, seed=3)]


TIE_PLACEMENTS = {"ends": 800, "adjacent": 800, "two_strides": 65536 + 600}     # kind -> n
_SHEAR = np.array([[2, 1, 0], [-1, 2, 1], [0, 1, 2]])          # integer, so the axes are not the coordinate axes
_TIE_CENTRES = {"right": np.array([42, 60, 72]), "left": np.array([40, 55, 30])}


def tie_slots(kind, n):
    """index pairs of the four extreme pairs (right axis 0, right axis 1, left axis 0, left axis 1)"""
    if kind == "ends":
        return [(k, n - 1 - k) for k in range(4)]                       # (0, n - 1) first
    if kind == "adjacent":
        return [(300 + 2 * k, 301 + 2 * k) for k in range(4)]           # (300, 301) first: one block, neighbouring threads
    return [(5 + k, 5 + k + 65536) for k in range(4)]                   # (5, 5 + 65 536): one thread, two strides


def tie_case(kind, minus_first: bool) -> PlateauCase:
    """Per plateau a set of small integers exactly symmetric about an integer centre, {c + p} u {c - p}: the mean is c exactly and
    mirrored points score exactly opposite on every axis.  Per plateau and axis one mirrored pair is the only extreme, at the indices
    ``tie_slots`` names; ``minus_first`` puts c - p at the earlier one.  The rule: the earlier index scores positive."""
    n = TIE_PLACEMENTS[kind]
    rng = np.random.default_rng(SEED + 300)
    v = np.zeros((n, 3), np.int64)
    slots = tie_slots(kind, n)
    free = np.setdiff1d(np.arange(n), np.array(slots).ravel())
    free = free[rng.permutation(len(free))]
    half = len(free) // 4
    for s, side in enumerate(("right", "left")):
        c = _TIE_CENTRES[side]
        q = np.stack([rng.integers(-6, 7, half), rng.integers(-2, 3, half), rng.integers(-1, 2, half)], axis=1) @ _SHEAR.T
        mine = free[2 * s * half:2 * (s + 1) * half]
        v[mine[:half]], v[mine[half:]] = c + q, c - q
        for axis, extreme in enumerate(((9, 0, 0), (0, 7, 0))):
            p = _SHEAR @ np.array(extreme)
            first, second = slots[2 * s + axis]
            v[first], v[second] = (c - p, c + p) if minus_first else (c + p, c - p)
    assert len(free) == 4 * half
    name = f"tie_{kind}_{'minus' if minus_first else 'plus'}_first"
    return PlateauCase(name, v.astype(np.float32), rng.uniform(0.5, 3.0, n).astype(np.float32))


def tie_cases():
    return [tie_case(kind, m) for kind in TIE_PLACEMENTS for m in (False, True)]


def scatter_eigenvalues(v):
    """descending eigenvalues of the centred 3x3 scatter matrix"""
    d = np.asarray(v, np.float64)
    d = d - d.mean(axis=0)
    return np.linalg.eigvalsh(d.T @ d)[::-1]
