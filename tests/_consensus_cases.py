"""The fixed inputs of the consensus tests (tests/test_consensus_oracle_cpu.py, tests/test_gpu_consensus.py): seeded cluster
samples, disjoint and overlapping, and the sample counts that put S K at the edges of the similarity kernel's loop."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from tests._align_cases import planted, relabelled_runs  # noqa: F401  (re-exported: the planted structures of the alignment tests)

GOLDEN = Path(__file__).resolve().parent / "golden"
STEP, ROUND = 64, 256                    # contraction elements per MFMA and per round of the loop (SBE_CONSENSUS_ROUND)
NS, KS = (1, 31, 32, 33, 64, 65, 257), (1, 3, 8)


def edge_lengths(k):
    """Sample counts S with S K just below, at and just above a step (64) and a round (256), and S = 1."""
    out = {1}
    for edge in (STEP, ROUND):
        out |= {max(1, (edge - 1) // k), -(-edge // k), -(-(edge + 1) // k)}
    return sorted(out)


def overlapping(s, k, n, seed, density=0.3):
    """uint8 [S, K, N]: independent bits, so objects sit in several areas of a sample and some rows are empty."""
    return (np.random.default_rng(seed).random((s, k, n)) < density).astype(np.uint8)


def disjoint(s, k, n, seed, outside=0.4):
    """uint8 [S, K, N]: every object in at most one area per sample."""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, k, (s, n))
    label[rng.random((s, n)) < outside] = -1
    return (label[:, None, :] == np.arange(k)[None, :, None]).astype(np.uint8)


def golden_realign():
    """tag -> (samples as logged, the same samples with every sample's labels permuted by the reference's realignment):
    uint8 [S, K, N] pairs of tests/golden/align.npz (bit-packed along the objects there)."""
    g = np.load(GOLDEN / "align.npz")
    out = {}
    for tag in ("k3_n100", "k5_n33"):
        s, k, n = (int(v) for v in g[f"realign_{tag}_shape"])
        out[tag] = tuple(np.unpackbits(g[f"realign_{tag}_{io}"], axis=-1)[:, :, :n].reshape(s, k, n) for io in ("in", "out"))
    return out


def three_runs():
    """Three runs of one planted structure (K = 4, N = 100) of different lengths, each with labels of its own."""
    return relabelled_runs(4, 100, [40, 33, 48], [[0, 1, 2, 3], [3, 1, 0, 2], [1, 2, 3, 0]], seed=1900)
