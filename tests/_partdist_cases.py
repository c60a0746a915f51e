"""The fixed inputs of the partition-distance tests (tests/test_partdist_oracle_cpu.py, tests/test_gpu_partdist.py,
tests/test_gpu_partdist_range.py): the consensus tests' seeded samples with disjoint areas, and the sample counts that put
T K_pad at the edges of the tile kernel's 32-row tiles.  A plain helper module: it holds no test."""
from __future__ import annotations

import numpy as np

from tests import _consensus_cases as consensus_cases
from tests._consensus_cases import disjoint  # noqa: F401  (re-exported)

NS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
KS = (1, 2, 3, 5, 8)                     # K_pad 1, 2, 4, 8, 8
TILE = 32


def padded(k):
    return 1 << (k - 1).bit_length()


def edge_lengths(k):
    """Sample counts T with T K_pad just below, at and just above one tile (32 rows) and two (64)."""
    per_tile = TILE // padded(k)
    out = set()
    for tiles in (1, 2):
        out |= {max(1, tiles * per_tile - 1), tiles * per_tile, tiles * per_tile + 1}
    return sorted(out)


def exclusive(samples):
    """The samples with every object kept only where exactly one area holds it: disjoint areas, and the same partition
    whatever the order of the labels (the planted and recorded samples below flip bits independently, so a few objects sit
    in several areas)."""
    c = np.asarray(samples).astype(np.uint8)
    return c * (c.sum(axis=1, keepdims=True) == 1).astype(np.uint8)


def three_runs():
    """_consensus_cases.three_runs() with disjoint areas: three runs of one planted structure (K = 4, N = 100) of 40, 33 and
    48 samples, each with labels of its own."""
    return [exclusive(r) for r in consensus_cases.three_runs()]


def golden_realign():
    """_consensus_cases.golden_realign() with disjoint areas: tag -> (samples as logged, the same samples under the labels
    of the reference's realignment)."""
    return {tag: (exclusive(a), exclusive(b)) for tag, (a, b) in consensus_cases.golden_realign().items()}


def labels_of(samples):
    """int64 [S, N]: the block of every object, 0 for no area and k + 1 for area k."""
    c = np.asarray(samples).astype(np.int64)
    return (c * np.arange(1, c.shape[1] + 1)[None, :, None]).sum(axis=1)


def position():
    """N = 321, K = 1, 322 samples: sample i < 321 is {i}, sample 321 is every object.  Every (round, step, lane half, dword,
    nibble) of the image's rows is hit by exactly one sample."""
    n = 321
    c = np.zeros((n + 1, 1, n), dtype=np.uint8)
    c[np.arange(n), 0, np.arange(n)] = 1
    c[n, 0, :] = 1
    return c


def limit():
    """N = 16384, K = 8, four samples: all objects in area 0, all in area 1, none clustered, and a split."""
    n = 16384
    c = np.zeros((4, 8, n), dtype=np.uint8)
    c[0, 0, :] = 1
    c[1, 1, :] = 1
    c[3, 2, :n // 2] = 1
    c[3, 7, n // 2:] = 1
    return c
