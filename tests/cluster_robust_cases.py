"""The cases of the cluster-robust regression (include/oai_hip.h, "Cluster-robust regression"): the shapes, the fixtures of
tests/cluster_robust_ref.py's ``hostile_case`` and their restatement.  tests/test_cluster_robust_cpu.py holds the restatement to
independent code on them, tests/test_cluster_robust_gpu.py holds the device to the restatement bit for bit.  No tests and no fixtures here."""
import functools

import cluster_robust_ref as cref

COLUMNS = (1, 2, 4, 6)                            # p: x alone; the intercept; two sizes of the kernel's rows per thread
VERTS = (1, 63, 65, 257)                          # both sides of a wave (64) and of a block's 256 vertices
KINDS = ("singletons", "two", "five", "word")


def counts_of(kind, p):
    """Rows per cluster.  singletons: one row per cluster; two: S = 2; five: S = 5, unbalanced, with single-visit clusters; word: S = 33,
    one more than a flip word holds.  Every shape leaves n - p >= 1 at an ordinary vertex."""
    return {"singletons": (1,) * (p + 6), "two": (p + 3, p + 1), "five": (1, p + 2, 1, 3, p),
            "word": tuple(1 + (s % 3) for s in range(33))}[kind]


def rows_per_thread(p):                           # csrc/cluster_robust.hip, rows_per_thread
    return {1: 16, 2: 16, 4: 16, 6: 8}[p]


def row_counts(p):
    """Flip rows: one fewer and one more than a thread owns, and two full groups and a ragged one."""
    r = rows_per_thread(p)
    return (r - 1, r + 1, 2 * r + 5)


@functools.lru_cache(maxsize=None)
def case(kind, V, p, masked):
    counts = counts_of(kind, p)
    Y, mask, D, offsets = cref.hostile_case(11, V, counts, masked, p)
    flips = cref.flip_rows(11, len(counts), max(row_counts(p)))
    flips.setflags(write=False)
    return Y, mask, D, offsets, flips


@functools.lru_cache(maxsize=None)
def reference(kind, V, p, masked):
    Y, mask, D, offsets, flips = case(kind, V, p, masked)
    block = cref.prepare(Y, mask, D, offsets, centre=p > 1)
    t, slope0, se0 = cref.cluster_t(block, flips, with_row0=True)
    for a in (t, slope0, se0):
        a.setflags(write=False)
    return block, t, slope0, se0
