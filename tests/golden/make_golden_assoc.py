#!/usr/bin/env python3
"""Record what the screening loop of the reference's find_correlated_features tool computes per pair of features:
`pd.crosstab` of the two state columns and `scipy.stats.chi2_contingency` on the table (the two library calls of the
loop body, made directly: the tool itself needs plotting packages).  Writes tests/golden/assoc.npz.

Runs only in the build container (needs pandas, SciPy and, for the south_america case, the reference's features.csv).
Per case `<c>`: `<c>_x` uint8 [N, F] state codes (255 = not observed; states numbered in sorted order), `<c>_n_states`
int32 [F], and over the pairs i < j in the tool's order (combinations): `<c>_statistic`, `<c>_pvalue` (float64; NaN
where skipped), `<c>_dof`, `<c>_n` (int32) and `<c>_skipped` (bool: the tool's `min(crosstab.shape) <= 1`).
Deterministic: every synthetic case is drawn from its own seeded generator.

    python tests/golden/make_golden_assoc.py            # rewrites tests/golden/assoc.npz
"""
import os
import sys
from itertools import combinations
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
OUT = Path(os.environ.get("SBAYES_AMD_GOLDEN_OUT", str(HERE)))
SOUTH_AMERICA_CSV = Path("/root/reference/experiments/south_america/data/features.csv")
NA = 255


def south_america():
    from sbayes_amd.assoc import frame_codes, read_features_csv
    codes, n_states, _names, _states = frame_codes(read_features_csv(SOUTH_AMERICA_CSV))
    return codes, n_states


def with_na(rng, x, frac):
    x = x.copy()
    x[rng.random(x.shape) < frac] = NA
    return x


def ragged(seed=101, n=300, f=40):
    """Ragged 2..10 states, 10 % NA, correlated blocks, and conditional features: observed only where another feature
    holds one state -- so that over their overlap that feature has a single state and the tool skips the pair."""
    rng = np.random.default_rng(seed)
    n_states = rng.integers(2, 11, size=f).astype(np.int32)
    x = np.stack([rng.integers(0, s, size=n) for s in n_states], axis=1).astype(np.uint8)
    for k in range(1, f, 5):                                 # dependence: follow the neighbour most of the time
        follow = rng.random(n) < 0.6
        x[follow, k] = x[follow, k - 1] % n_states[k]
    x = with_na(rng, x, 0.10)
    for k in range(3, f, 7):                                 # conditional on feature k - 2 holding its state 0
        x[x[:, k - 2] != 0, k] = NA
    return x, n_states


def binary(seed=102, n=1000, f=64):
    rng = np.random.default_rng(seed)
    base = rng.random((n, 8)) < 0.5
    mix = rng.integers(0, 8, size=f)
    noise = rng.random((n, f)) < rng.uniform(0.05, 0.5, size=f)[None, :]
    x = (base[:, mix] ^ noise).astype(np.uint8)
    return with_na(rng, x, 0.05), np.full(f, 2, dtype=np.int32)


def duplicated(seed=103, n=5000, s=10):
    """A feature and its copy (p-value underflows to 0 in SciPy), a noisy copy and an independent one."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, s, size=n)
    noisy = np.where(rng.random(n) < 0.5, a, rng.integers(0, s, size=n))
    x = np.stack([a, a, noisy, rng.integers(0, s, size=n)], axis=1).astype(np.uint8)
    return x, np.full(4, s, dtype=np.int32)


def edge_s32(seed=104):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 32, size=700)
    b = np.where(rng.random(700) < 0.2, a, rng.integers(0, 32, size=700))
    x = np.stack([a, b, rng.integers(0, 32, size=700)], axis=1).astype(np.uint8)
    return with_na(rng, x, 0.05), np.full(3, 32, dtype=np.int32)


def edge_one_object():
    return np.array([[0, 1, NA]], dtype=np.uint8), np.array([2, 3, 2], dtype=np.int32)


def edge_ragged_n(seed=105):
    """N = 131 (no multiple of 64), one feature NA everywhere, one with a single state."""
    rng = np.random.default_rng(seed)
    n_states = np.array([2, 3, 5, 2, 4, 2], dtype=np.int32)
    x = np.stack([rng.integers(0, s, size=131) for s in n_states], axis=1).astype(np.uint8)
    x = with_na(rng, x, 0.15)
    x[:, 3] = NA
    x[x[:, 5] != NA, 5] = 1
    return x, n_states


def edge_two_features(seed=106):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, size=64)
    return np.stack([a, a ^ (rng.random(64) < 0.2)], axis=1).astype(np.uint8), np.array([2, 2], dtype=np.int32)


CASES = {
    "south_america": south_america,
    "ragged": ragged,
    "binary": binary,
    "duplicated": duplicated,
    "edge_s32": edge_s32,
    "edge_one_object": edge_one_object,
    "edge_ragged_n": edge_ragged_n,
    "edge_two_features": edge_two_features,
}


def screen(x):
    """The loop body of the tool over all pairs of the code matrix."""
    import pandas as pd
    from scipy.stats import chi2_contingency
    frame = pd.DataFrame({f"F{k}": [None if c == NA else f"s{c:02d}" for c in x[:, k]] for k in range(x.shape[1])}, dtype=object)
    stat, pval, dof, n, skipped = [], [], [], [], []
    for f1, f2 in combinations(frame.columns, 2):
        crosstab = pd.crosstab(frame[f1], frame[f2])
        n.append(int(crosstab.to_numpy().sum()))
        if min(crosstab.shape) <= 1:
            stat.append(0.0), pval.append(np.nan), dof.append(0), skipped.append(True)
            continue
        res = chi2_contingency(crosstab)
        stat.append(float(res.statistic)), pval.append(float(res.pvalue)), dof.append(int(res.dof)), skipped.append(False)
    return (np.array(stat, dtype=np.float64), np.array(pval, dtype=np.float64), np.array(dof, dtype=np.int32),
            np.array(n, dtype=np.int32), np.array(skipped, dtype=np.bool_))


def main():
    out = {}
    for name, make in CASES.items():
        x, n_states = make()
        stat, pval, dof, n, skipped = screen(x)
        out.update({f"{name}_x": x, f"{name}_n_states": n_states, f"{name}_statistic": stat, f"{name}_pvalue": pval,
                    f"{name}_dof": dof, f"{name}_n": n, f"{name}_skipped": skipped})
        print(f"{name}: N={x.shape[0]} F={x.shape[1]} pairs={len(stat)} skipped={int(skipped.sum())} dof1={int((dof == 1).sum())} "
              f"below 1e-4: {int(np.sum(pval < 1e-4))} min p={np.nanmin(pval) if (~skipped).any() else float('nan'):.3g}")
    np.savez_compressed(OUT / "assoc.npz", **out)


if __name__ == "__main__":
    main()
