"""The fixed inputs of the partition-search tests (tests/test_partsearch_oracle_cpu.py, tests/test_gpu_partsearch.py): seeded
noisy samples of a planted partition as label rows, the starts of a search as sbayes_amd.partsearch makes them, the
brute-force set and the shapes at the strides of the tree.  A plain helper module: it holds no test."""
from __future__ import annotations

import itertools

import numpy as np

from sbayes_amd import partsearch
from tests import _partsearch_oracle as orc

# (N, K, T, starts): every N, K, T and start count at which the kernels take another path -- T at the lane and thread strides
# of the tree, N around the transpose's tile of 32 and past one block of 256 objects, one and several workgroups
GRID = [(1, 1, 1, 1), (2, 2, 2, 3), (31, 5, 63, 3), (32, 8, 64, 1), (33, 1, 65, 3), (257, 2, 255, 1), (31, 8, 256, 3), (33, 5, 257, 3),
        (257, 8, 513, 1), (33, 2, 65, 65)]
LOSSES = ("vi", "binder")
BRUTE_SEEDS = tuple(range(28))           # N = 7, K = 2: all 3^7 candidates are enumerated


def noisy(seed, n, k, t, flip=0.25, labels=None):
    """(y uint8 [T, N], truth uint8 [N]): a planted partition with labels drawn from `labels` (default 0..K), and per sample
    a share `flip` of the objects relabelled uniformly."""
    rng = np.random.default_rng(seed)
    pool = np.arange(k + 1) if labels is None else np.asarray(labels)
    truth = pool[rng.integers(0, len(pool), size=n)].astype(np.uint8)
    y = np.repeat(truth[None], t, axis=0)
    scrambled = rng.random((t, n)) < flip
    y[scrambled] = pool[rng.integers(0, len(pool), size=int(scrambled.sum()))]
    return y, truth


def medoid_of(y, k, loss):
    """The sample with the smallest (loss sum, index), by the checker."""
    _, _, vi_sum, binder_sum = orc.evaluate(y, y, k)
    return int(np.argmin(vi_sum if loss == "vi" else binder_sum))


def starts_of(y, k, starts, seed, loss="vi"):
    """(init, order) as sbayes_amd.partsearch.search makes them."""
    init, order, _ = partsearch.make_starts(y, medoid_of(y, k, loss), k, starts, seed)
    return init, order


def random_starts(seed, n, k, starts):
    """(init, order): uniform random labellings under random permutations."""
    rng = np.random.default_rng(seed)
    init = rng.integers(0, k + 1, size=(starts, n)).astype(np.uint8)
    order = np.stack([rng.permutation(n) for _ in range(starts)]).astype(np.int32)
    return init, order


def oracle_starts(y, k, loss, init, order, max_sweeps):
    return [orc.search(y, k, loss, init[s], order[s], max_sweeps) for s in range(init.shape[0])]


def brute(seed):
    """y uint8 [12, 7], K = 2."""
    return noisy(1000 + seed, 7, 2, 12, flip=0.3)[0], 2


def brute_force(y, k):
    """(vi_sum float64, binder_sum int64) of every candidate in 0..K ^ N, in plain NumPy (the order of the VI sums is not
    the contract's)."""
    t, n = y.shape
    cands = np.array(list(itertools.product(range(k + 1), repeat=n)), dtype=np.int64)
    eye = np.eye(k + 1, dtype=np.int64)
    e = np.einsum("ciq,til->ctql", eye[cands], eye[y.astype(np.int64)])
    table = orc.xlogx(n)
    a, b = e.sum(axis=3), e.sum(axis=2)
    vi = (table[a].sum(axis=2) + table[b].sum(axis=2) - 2.0 * table[e].sum(axis=(2, 3))) / n
    binder = (a[:, :, 1:] ** 2).sum(axis=2) + (b[:, :, 1:] ** 2).sum(axis=2) - 2 * (e[:, :, 1:, 1:] ** 2).sum(axis=(2, 3))
    return cands, vi.sum(axis=1), binder.sum(axis=1)


def contradictory():
    """T = 2 samples of N = 6 objects, K = 2, that contradict each other: under Binder's loss an object scores the same in
    several blocks, so both branches of the tie rule are taken (the CPU tests assert that they are)."""
    y = np.array([[1, 1, 1, 2, 2, 0], [2, 1, 2, 1, 2, 1]], dtype=np.uint8)
    init = np.array([[1, 1, 1, 2, 2, 0], [0, 0, 0, 0, 0, 0], [2, 2, 1, 1, 0, 2]], dtype=np.uint8)
    order = np.stack([np.arange(6), np.arange(6)[::-1], np.array([3, 0, 5, 1, 4, 2])]).astype(np.int32)
    return y, 2, init, order
