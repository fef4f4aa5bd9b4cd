"""A numpy restatement of csrc/ordered_reduce.h in plain fp64: the order in which the QC kernels add up.  IEEE add, fmin and fmax on
numpy float64 are bit-faithful, so a sum restated here equals the device's bit for bit, and a reordering on the device shows.

An accumulator is an array [..., N] with a tuple of N operations ("add", "min", "max") and its cleared value."""
import functools
import math

import numpy as np

KT, WAVE = 256, 64
_OPS = {"add": np.add, "min": np.fmin, "max": np.fmax}

# SurfAcc of csrc/edt.hip: n_A, n_B, sum d(A->B), sum d(B->A), max d(A->B), max d(B->A)
SURF_OPS = ("add", "add", "add", "add", "max", "max")
SURF_CLEAR = np.array([0.0, 0.0, 0.0, 0.0, -np.inf, -np.inf])
STREAM_BLOCKS = 2048                       # kStreamBlocks

# n = 1, 63, 64, 65, 1025: partial waves and one or two blocks; more than 256 slots: the finish takes runs of two; the grid-stride
# cap: threads take two elements
ORDER_SIZES = (1, 63, 64, 65, 1025, 1024 * 257 + 3, 2048 * 1024 + 5)
ORDER_SEED = 7


def merge(a, b, ops):
    """a (the earlier elements) on the left of every operation."""
    return np.stack([_OPS[op](a[..., i], b[..., i]) for i, op in enumerate(ops)], axis=-1)


def block_reduce(v, ops):
    """[..., KT, N] per-thread accumulators -> [..., N]: block_reduce of the header, as thread 0 sees it."""
    v = np.array(v, dtype=np.float64).reshape(v.shape[:-2] + (KT // WAVE, WAVE, v.shape[-1]))
    off = WAVE // 2
    while off >= 1:                        # v[l] = merge(v[l], v[l + off]) for l + off < 64, all lanes at once; only lane 0's cone matters
        v[..., : WAVE - off, :] = merge(v[..., : WAVE - off, :], v[..., off:, :], ops)
        off //= 2
    r = v[..., 0, 0, :]
    for w in range(1, KT // WAVE):         # the waves in order
        r = merge(r, v[..., w, 0, :], ops)
    return r


def reduce_slots(partials, clear, ops):
    """[nb, N] slots -> [KT, N]: thread t merges slots [t per, min((t + 1) per, nb)) serially into a cleared accumulator."""
    nb = partials.shape[0]
    per = -(-nb // KT)
    acc = np.tile(np.asarray(clear, np.float64), (KT, 1))
    for j in range(per):
        idx = np.arange(KT) * per + j
        ok = idx < nb
        acc[ok] = merge(acc[ok], partials[idx[ok]], ops)
    return acc


def finish(partials, clear, ops):
    """The one-block finish kernel: the slots in runs, then the same tree."""
    return block_reduce(reduce_slots(partials, clear, ops), ops)


def surface_stats(sa, db, sb, da):
    """out[0..5] of oai_surface_distance driven the way surface_partials_kernel is: blocks = min(2048, ceil(n / 1024)), thread
    b 256 + t takes i = b 256 + t, + blocks 256, ...; each term is (double)float32."""
    n = sa.size
    blocks = max(1, min(STREAM_BLOCKS, -(-n // (4 * KT))))
    threads = blocks * KT
    acc = np.tile(SURF_CLEAR, (threads, 1))
    for start in range(0, n, threads):
        m = min(threads, n - start)
        for mask, dist, k in ((sa, db, 0), (sb, da, 1)):
            on = np.flatnonzero(mask[start:start + m])
            d = dist[start:start + m][on].astype(np.float64)
            acc[on, k] = acc[on, k] + 1.0
            acc[on, 2 + k] = acc[on, 2 + k] + d
            acc[on, 4 + k] = np.fmax(acc[on, 4 + k], d)
    return finish(block_reduce(acc.reshape(blocks, KT, 6), SURF_OPS), SURF_CLEAR, SURF_OPS)


@functools.lru_cache(maxsize=None)
def order_case(n, seed=ORDER_SEED):
    """1-D inputs of oai_surface_distance on which the order shows: random masks of density 0.3 (element 0 in both, so that no
    surface is empty) and float32 distances exp(U(-20, 20)); with them the restated figures and, per direction, the terms in index
    order, their exactly rounded sum and their plain left-to-right sum."""
    rng = np.random.default_rng([seed, n])
    sa, sb = ((rng.uniform(size=n) < 0.3).astype(np.uint8) for _ in range(2))
    sa[0] = sb[0] = 1
    db, da = (np.exp(rng.uniform(-20.0, 20.0, size=n)).astype(np.float32) for _ in range(2))
    want = surface_stats(sa, db, sb, da)
    terms = [db[sa != 0].astype(np.float64), da[sb != 0].astype(np.float64)]
    exact = [math.fsum(t) for t in terms]
    serial = [float(np.add.accumulate(t)[-1]) for t in terms]
    for a in (sa, db, sb, da, want, *terms):
        a.setflags(write=False)
    return (sa, db, sb, da), want, terms, exact, serial
