"""The fixed inputs of the similarity-error tests (tests/test_simerr_oracle_cpu.py, tests/test_gpu_simerr.py): seeded cluster
samples, the planted degenerate cases, the shapes that put b K at the edges of a step, and the chains of the estimator checks."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from tests._consensus_cases import disjoint, overlapping  # noqa: F401  (re-exported: the seeded samples of the consensus tests)

GOLDEN = Path(__file__).resolve().parent / "golden"
NS, KS = (1, 31, 32, 33, 65), (1, 3, 5, 8)
# (b, K) with b K = 1, 63, 64, 65, 128, 257, 320: below, at and above one step, two steps, one round of four steps and a step,
# and 560 = two rounds and a step
BATCH_SHAPES = ((1, 1), (21, 3), (63, 1), (8, 8), (13, 5), (16, 8), (257, 1), (64, 5), (40, 8), (70, 8))
THRESHOLDS = (3.84, 6.63, 10.83)


def planted(b=4, nb=3):
    """Two runs uint8 [nb b, 2, 9] of disjoint areas, and what they plant:
    objects 0, 1: in area 0 always, in both runs (V = 0 on both sides, equal P: z2 = 0);
    objects 2, 8: in area 0 always in run a, in area 1 always in run b (against 0: V = 0 on both sides, P = 1 and 0: inf,
                  attained at columns 2 and 8 of rows 0 and 1: tied maxima);
    object 3: in no area (all-zero rows); object 4: in both areas always (an all-ones column: its counts are b or 2 b per batch);
    objects 5, 6: one seeded membership for both, of its own in each run; object 7: in area 1 in the samples of batch 1 of
                  run a and nowhere else (with object 4: together in exactly one batch)."""
    rng = np.random.default_rng(7100)
    runs = []
    for r in range(2):
        c = np.zeros((nb * b, 2, 9), dtype=np.uint8)
        c[:, 0, [0, 1]] = 1
        c[:, r, [2, 8]] = 1
        c[:, :, 4] = 1
        where = rng.integers(0, 3, nb * b)                     # area 0, area 1 or none
        for s, w in enumerate(where):
            if w < 2:
                c[s, w, [5, 6]] = 1
        if r == 0:
            c[b:2 * b, 1, 7] = 1
        runs.append(c)
    return runs


def independent(n_samples, k, n, seed):
    """uint8 [S, K, N]: every object draws one of K labels uniformly, every sample anew."""
    label = np.random.default_rng(seed).integers(0, k, (n_samples, n))
    return (label[:, None, :] == np.arange(k)[None, :, None]).astype(np.uint8)


def sticky(n_samples, k, n, seed, keep=0.9):
    """uint8 [S, K, N]: a chain in which every object keeps its label with probability `keep` and else draws a new one
    uniformly from all K."""
    rng = np.random.default_rng(seed)
    label = np.empty((n_samples, n), dtype=np.int64)
    label[0] = rng.integers(0, k, n)
    for s in range(1, n_samples):
        fresh = rng.integers(0, k, n)
        label[s] = np.where(rng.random(n) < keep, label[s - 1], fresh)
    return (label[:, None, :] == np.arange(k)[None, :, None]).astype(np.uint8)


def diag_runs():
    """The two recorded runs of tests/golden/diag_runs.npz: uint8 [60, K, N] each."""
    g = np.load(GOLDEN / "diag_runs.npz")
    kn = int(g["n_cluster_columns"])
    k = 1 + int(str(g["cluster_names"][-1]).split("_")[0][1:])
    return [np.unpackbits(g[f"clusters_{r}"], axis=1)[:, :kn].reshape(-1, k, kn // k) for r in range(2)]


def limit_run(n_batches=1 << 10, b=1 << 10):
    """uint8 [n_batches b, 8, 2] for the store at the accumulator's limit: object 0 in every area of every sample, object 1 in
    every area of the first q + 1 samples of batch q.  Per batch c_q[0][0] = 8 b, c_q[0][1] = c_q[1][1] = 8 (q + 1)."""
    s = np.arange(n_batches * b)
    rows = np.ones((n_batches * b, 8, 2), dtype=np.uint8)
    rows[:, :, 1] = (s % b <= s // b)[:, None]
    return rows


def limit_moments(n_runs, n_batches=1 << 10, b=1 << 10):
    """(S1, S2, nB) of n_runs such runs in closed form: Python integers [2][2]."""
    m = n_batches
    first, squares = m * (m + 1) // 2, m * (m + 1) * (2 * m + 1) // 6
    s1 = [[n_runs * 8 * b * m, n_runs * 8 * first], [n_runs * 8 * first, n_runs * 8 * first]]
    s2 = [[n_runs * 64 * b * b * m, n_runs * 64 * squares], [n_runs * 64 * squares, n_runs * 64 * squares]]
    return s1, s2, n_runs * m
