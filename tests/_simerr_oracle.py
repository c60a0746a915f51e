"""The checker of sbayes_amd.simerr: the contract of include/sbe_simerr.h restated in NumPy, integers in exact int64.

Runs are 0/1 arrays [S_r, K, N]; b is the batch length.  Batch q of a run is its samples [q b, (q + 1) b); a trailing
incomplete batch is not used.  For a side (a list of runs) with nB complete batches in all, Z_q the cluster rows of batch q,
[b K, N]:
    c_q = Z_q^T Z_q                              the rows of the batch that hold both i and j (integer matmul)
    S1 = sum_q c_q      S2 = sum_q c_q^2        V = nB S2 - S1^2 >= 0
    P = S1 / (nB b)     se^2 = V / (nB^2 (nB - 1) b^2)
    compare (a against b)   D = S1_a nB_b - S1_b nB_a
                            z2 = D^2 / (nB_b^2 V_a / (nB_a - 1) + nB_a^2 V_b / (nB_b - 1))  in float64, in this order:
                                d = float(D); num = d * d
                                qa = (float(V_a) * float(nB_b nB_b)) / float(nB_a - 1); qb likewise; den = qa + qb
                                z2 = num / den if den > 0 else (0 if D == 0 else inf)
                            row_max = max_j z2, row_arg the smallest j that attains it, row_count[i][m] = #{j: z2 > thr[m]}
A side needs nB >= 2.  `moments_loops` and `z2_fraction` are a second route in plain Python integers and Fractions."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def batch_counts(runs, b):
    """int64 [nB, N, N]: c_q of every complete batch of the runs, in order."""
    out = []
    for run in runs:
        run = np.asarray(run)
        for q in range(run.shape[0] // b):
            z = run[q * b:(q + 1) * b].reshape(-1, run.shape[-1]).astype(np.int64)
            out.append(z.T @ z)
    n = np.asarray(runs[0]).shape[-1]
    return np.stack(out) if out else np.zeros((0, n, n), dtype=np.int64)


def moments(runs, b):
    """(S1, S2, nB): int64 [N, N] each and the number of complete batches."""
    c = batch_counts(runs, b)
    if c.shape[0] < 2:
        raise ValueError(f"{c.shape[0]} complete batches; a side takes at least 2")
    return c.sum(axis=0), (c * c).sum(axis=0), int(c.shape[0])


def variance(s1, s2, nb):
    v = int(nb) * np.asarray(s2, dtype=np.int64) - np.asarray(s1, dtype=np.int64) ** 2
    assert (v >= 0).all()
    return v


def probability(s1, nb, b):
    return np.asarray(s1) / float(nb * b)


def se_squared(s1, s2, nb, b):
    return variance(s1, s2, nb).astype(np.float64) / float(nb * nb * (nb - 1) * b * b)


def z2(side_a, side_b):
    """float64 [N, N] from two (S1, S2, nB)."""
    (s1a, s2a, nba), (s1b, s2b, nbb) = side_a, side_b
    va, vb = variance(s1a, s2a, nba), variance(s1b, s2b, nbb)
    diff = np.asarray(s1a, dtype=np.int64) * nbb - np.asarray(s1b, dtype=np.int64) * nba
    d = diff.astype(np.float64)
    num = d * d
    qa = (va.astype(np.float64) * float(nbb * nbb)) / float(nba - 1)
    qb = (vb.astype(np.float64) * float(nba * nba)) / float(nbb - 1)
    den = qa + qb
    out = np.empty(diff.shape, dtype=np.float64)
    for at in np.ndindex(*diff.shape):                          # (plain branches: no warning to silence, no where to trust)
        out[at] = num[at] / den[at] if den[at] > 0.0 else (0.0 if diff[at] == 0 else np.inf)
    return out


def compare(side_a, side_b, thresholds=()):
    """(z2 [N, N], row_max [N], row_arg int32 [N], row_count int32 [N, M])."""
    z = z2(side_a, side_b)
    row_max = z.max(axis=1)
    row_arg = np.array([int(np.flatnonzero(row == m)[0]) for row, m in zip(z, row_max)], dtype=np.int32)
    row_count = np.array([[int(np.count_nonzero(row > t)) for t in thresholds] for row in z], dtype=np.int32).reshape(z.shape[0], len(thresholds))
    return z, row_max, row_arg, row_count


# ---- the second route: Python integers over explicit loops, exact rationals -----------------------------------------------
def moments_loops(runs, b):
    """(S1, S2, nB) as nested lists of Python integers, by the definition."""
    n = len(runs[0][0][0])
    s1 = [[0] * n for _ in range(n)]
    s2 = [[0] * n for _ in range(n)]
    nb = 0
    for run in runs:
        for q in range(len(run) // b):
            nb += 1
            for i in range(n):
                for j in range(n):
                    c = 0
                    for s in range(q * b, (q + 1) * b):
                        for row in run[s]:
                            c += int(row[i]) * int(row[j])
                    s1[i][j] += c
                    s2[i][j] += c * c
    return s1, s2, nb


def z2_fraction(s1a, s2a, nba, s1b, s2b, nbb):
    """z2 of one entry as an exact Fraction, or 0 / 'inf' in the degenerate cases."""
    va, vb = nba * s2a - s1a * s1a, nbb * s2b - s1b * s1b
    d = s1a * nbb - s1b * nba
    den = Fraction(nbb * nbb * va, nba - 1) + Fraction(nba * nba * vb, nbb - 1)
    if den > 0:
        return Fraction(d * d) / den
    return 0 if d == 0 else "inf"


# ---- the one-call functions ---------------------------------------------------------------------------------------------
def trim(runs, burnin, b):
    """The runs after burn-in (int(burnin S_r) leading samples) and without their leading S_r mod b samples."""
    out = []
    for run in runs:
        run = np.asarray(run)[int(burnin * len(run)):]
        out.append(run[len(run) % b:])
    return out


def default_batch_rows(runs, burnin):
    shortest = min(len(r) - int(burnin * len(r)) for r in runs)
    b = int(np.sqrt(shortest))
    while b * b > shortest:
        b -= 1
    while (b + 1) * (b + 1) <= shortest:
        b += 1
    return max(1, b)


def run_agreement(runs, b, thresholds):
    """Per pair a < c of (trimmed) runs: (max_z2, (i, j), shares over the pairs i <= j, max_abs, object_max)."""
    sides = [moments([r], b) for r in runs]
    n = sides[0][0].shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool))
    out = {}
    for a in range(len(runs)):
        for c in range(a + 1, len(runs)):
            z = z2(sides[a], sides[c])
            best = z.max()
            i, j = (int(v) for v in np.argwhere(upper & (z == best))[0])
            shares = [int(np.count_nonzero(z[upper] > t)) / int(upper.sum()) for t in thresholds]
            d = np.abs(sides[a][0] * sides[c][2] - sides[c][0] * sides[a][2])
            out[a, c] = (best, (i, j), shares, int(d.max()) / (sides[a][2] * sides[c][2] * b), z.max(axis=1))
    return out
