"""The fixed inputs of the alignment tests (tests/test_align_oracle_cpu.py, tests/test_gpu_align.py,
tests/golden/make_align_golden.py): cluster samples with planted blocks, label switching, noise and emptied clusters."""
from __future__ import annotations

import numpy as np

S_DEFAULT = 48
ORACLE_KS, ORACLE_NS = (2, 3, 5, 7), (33, 100, 257)
# seeds of the grid cases that replace 1000 + K * N: under the recipe's own seed a later step of the case has more
# than one optimal permutation (tests/test_align_oracle_cpu.py asserts the tie counts of every case)
RESEEDED = {}


def block_sizes(k, n):
    """K distinct block sizes over about half the objects: t, 2 t, ..., K t; where K (K + 1) / 2 > N the objects are
    dealt out evenly instead (sizes then repeat, some may be 0)."""
    least = k * (k + 1) // 2
    if least > n:
        return [n // k + (1 if i < n % k else 0) for i in range(k)]
    t = max(1, (n // 2) // least)
    return [t * (i + 1) for i in range(k)]


def planted(k, n, s=S_DEFAULT, flip=0.05, seed=None, shuffle=True, empty_every=7):
    """uint8 [S, K, N]: K disjoint planted blocks, every bit flipped with probability `flip` per sample, every
    `empty_every`-th sample with one cluster emptied, the rows of every sample shuffled by a random permutation.
    Returns (samples, the row shuffles [S, K]: sample s holds planted block shuffles[s][j] at row j)."""
    rng = np.random.default_rng(RESEEDED.get((k, n), 1000 + k * n) if seed is None else seed)
    base = np.zeros((k, n), dtype=np.uint8)
    at = 0
    for i, size in enumerate(block_sizes(k, n)):
        base[i, at:at + size] = 1
        at += size
    out = np.empty((s, k, n), dtype=np.uint8)
    shuffles = np.empty((s, k), dtype=np.int64)
    for t in range(s):
        c = base ^ (rng.random((k, n)) < flip).astype(np.uint8)
        if empty_every and t % empty_every == empty_every - 1:
            c[(t // empty_every) % k] = 0
        shuffles[t] = rng.permutation(k) if shuffle else np.arange(k)
        out[t] = c[shuffles[t]]
    return out, shuffles


def relabelled_runs(k, n, lengths, relabel, seed, flip=0.05, switch_every=0):
    """Runs of one planted structure: run r has noise of its own and its labels moved by relabel[r] (row j of its samples
    holds planted block relabel[r][j]); with switch_every, every switch_every-th sample has its rows shuffled on top."""
    runs = []
    for r, (length, q) in enumerate(zip(lengths, relabel)):
        c, _ = planted(k, n, length, flip, seed=seed + 17 * r, shuffle=False, empty_every=0)
        c = c[:, list(q)]
        if switch_every:
            rng = np.random.default_rng(seed + 17 * r + 5)
            for t in range(switch_every - 1, length, switch_every):
                c[t] = c[t][rng.permutation(k)]
        runs.append(np.ascontiguousarray(c))
    return runs


def dominant_blocks(k, n, counts):
    """The planted block each label of a count table [K, N] covers most."""
    edges = np.concatenate([[0], np.cumsum(block_sizes(k, n))])
    per_block = np.stack([np.asarray(counts)[:, edges[b]:edges[b + 1]].sum(axis=1) for b in range(k)], axis=1)
    return per_block.argmax(axis=1)


def tie_cases():
    """name -> uint8 [S, K, N]: inputs whose agreement matrices have several optimal permutations."""
    rng = np.random.default_rng(77)
    cases = {"all_zero": np.zeros((9, 4, 40), dtype=np.uint8)}
    twin, _ = planted(4, 65, 24, 0.05, seed=78)
    twin[:, 1] = twin[:, 0]
    cases["two_identical_clusters"] = twin
    empty, _ = planted(5, 70, 24, 0.05, seed=79)
    empty[:, 3] = 0
    empty[::2, 0] = 0
    cases["empty_clusters"] = empty
    cases["flip_0.2_n33"] = planted(5, 33, S_DEFAULT, 0.2, seed=80)[0]
    same = np.broadcast_to((rng.random((21, 1, 50)) < 0.3).astype(np.uint8), (21, 8, 50))
    cases["k8_every_cluster_equal"] = np.ascontiguousarray(same)
    return cases
