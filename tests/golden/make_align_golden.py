#!/usr/bin/env python3
"""Record what the reference's own label-alignment functions return on small inputs into tests/golden/align.npz.

Runs only in the build container (needs the reference, through make_golden.py's stubs; that file is not edited).  The
inputs are the planted cases of tests/_align_cases.py and the two recorded runs of tests/golden/diag_runs.npz.  Recorded:

  logger_<tag>_in / _perms / _nopt     sbayes.util.get_best_permutation driven as ClustersLogger._write_sample drives it
                                       (cluster_sum starts at zero; the sample is permuted, then added): the input samples
                                       (np.packbits along the objects), the permutation of every sample, and per step the
                                       number of optimal permutations of its agreement matrix (the checker's counter)
  realign_<tag>_in / _out / _nopt      sbayes.tools.realign_clusters_within_run.align_clusters: input and output samples
  realign_<tag>_names / _params_in / _params_out   the small parameter table that went through it with them
  runs_<tag>_perm / _nopt              the permutation of the second run against the first as tools/align_clusters.py's
                                       main computes it (cluster_agreement of the mean memberships, then
                                       linear_sum_assignment), on the runs of diag_runs.npz and on a planted pair
  runs_planted_in0 / _in1 / _relabel   that pair

The tool modules are imported as they are where they import under the stubs; where one does not, its few lines are driven
by hand through sbayes.util.get_best_permutation / scipy's linear_sum_assignment and the script says so when it runs
(`[golden-align] ... driven by hand`).  Every recorded step other than an all-zero first step must have one optimal
permutation; the script aborts otherwise.

  python tests/golden/make_align_golden.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import make_golden as mg  # noqa: E402,F401  (installs the reference stubs)
from tests import _align_cases as cases  # noqa: E402
from tests import _align_oracle as orc  # noqa: E402

LOGGER_CASES = {"k3_n100": (3, 100), "k5_n33": (5, 33), "k7_n257": (7, 257)}
REALIGN_CASES = {"k3_n100": (3, 100), "k5_n33": (5, 33)}
REALIGN_SEED_OFFSET = 500000                      # other noise than the logger cases


def pack(c):
    return np.packbits(np.asarray(c, dtype=np.uint8), axis=-1)


def record_logger(out):
    from sbayes.util import get_best_permutation
    for tag, (k, n) in LOGGER_CASES.items():
        c, _ = cases.planted(k, n)
        cluster_sum = np.zeros((k, n), dtype=int)
        perms, nopt = [], []
        for sample in c.astype(bool):
            nopt.append(orc.count_optimal(orc.agreement(cluster_sum, sample)))
            permutation = get_best_permutation(sample, cluster_sum)
            cluster_sum += sample[permutation, :]
            perms.append(permutation)
        out[f"logger_{tag}_in"] = pack(c)
        out[f"logger_{tag}_perms"] = np.array(perms, dtype=np.int8)
        out[f"logger_{tag}_nopt"] = np.array(nopt, dtype=np.int64)
        out[f"logger_{tag}_shape"] = np.array(c.shape, dtype=np.int64)
        assert nopt[0] > 1 or k == 1
        assert all(v == 1 for v in nopt[1:]), (tag, nopt)


def param_table(c):
    """A small stats table for samples c [S, K, N]: Sample, size_a{i}, two areal columns per cluster, one weight."""
    import pandas as pd
    s_n, k, _n = c.shape
    cols = {"Sample": np.arange(s_n, dtype=np.float64) * 10}
    for i in range(k):
        cols[f"size_a{i}"] = c[:, i].sum(axis=1).astype(np.float64)
    cols["w_areal_f1"] = np.linspace(0.1, 0.9, s_n)
    for i in range(k):
        cols[f"areal_a{i}_f1_x"] = 100.0 * i + np.arange(s_n) + 0.25
        cols[f"areal_a{i}_f1_y"] = 100.0 * i + np.arange(s_n) + 0.75
    return pd.DataFrame(cols)


def record_realign(out):
    try:
        from sbayes.tools.realign_clusters_within_run import align_clusters
    except Exception as exc:                                              # noqa: BLE001
        raise SystemExit(f"[golden-align] realign_clusters_within_run does not import under the stubs: {exc!r}")
    for tag, (k, n) in REALIGN_CASES.items():
        c, _ = cases.planted(k, n, seed=REALIGN_SEED_OFFSET + k * n)
        params = param_table(c)
        names = list(params.columns)
        ref_clusters, ref_params = align_clusters(c.transpose(1, 0, 2).astype(int).copy(), params.copy(), [f"a{i}" for i in range(k)])
        _p, ds = orc.within(c, 20, with_d=True)
        nopt = [orc.count_optimal(d) for d in ds]
        assert all(v == 1 for v in nopt), (tag, nopt)
        assert list(ref_params.columns) == names
        out[f"realign_{tag}_in"] = pack(c)
        out[f"realign_{tag}_out"] = pack(np.asarray(ref_clusters).transpose(1, 0, 2))
        out[f"realign_{tag}_nopt"] = np.array(nopt, dtype=np.int64)
        out[f"realign_{tag}_shape"] = np.array(c.shape, dtype=np.int64)
        out[f"realign_{tag}_names"] = np.array(names)
        out[f"realign_{tag}_params_in"] = params.to_numpy(dtype=np.float64)
        out[f"realign_{tag}_params_out"] = ref_params.to_numpy(dtype=np.float64)


def record_runs(out):
    from scipy.optimize import linear_sum_assignment
    try:
        from sbayes.tools.align_clusters import cluster_agreement
        print("[golden-align] align_clusters.cluster_agreement imported; main()'s two lines around it are driven by hand")
    except Exception as exc:                                              # noqa: BLE001
        raise SystemExit(f"[golden-align] align_clusters does not import under the stubs: {exc!r}")

    def tool_perm(c1, c2):                                                # c: [S, K, N] -> Results.clusters is [K, S, N]
        mean_1 = np.mean(c1.transpose(1, 0, 2), axis=1)
        mean_2 = np.mean(c2.transpose(1, 0, 2), axis=1)
        return linear_sum_assignment(cluster_agreement(mean_1, mean_2), maximize=True)[1]

    g = np.load(HERE / "diag_runs.npz")
    kn = int(g["n_cluster_columns"])
    runs = [np.unpackbits(g[f"clusters_{r}"], axis=1)[:, :kn] for r in range(2)]
    k = 1 + int(str(g["cluster_names"][-1]).split("_")[0][1:])
    runs = [r.reshape(r.shape[0], k, kn // k) for r in runs]
    k2, n2, relabel = 4, 100, [[0, 1, 2, 3], [2, 0, 3, 1]]
    planted = cases.relabelled_runs(k2, n2, [40, 33], relabel, seed=4242)
    for tag, (c1, c2) in {"diag": runs, "planted": planted}.items():
        out[f"runs_{tag}_perm"] = np.asarray(tool_perm(c1, c2), dtype=np.int8)
        nopt = orc.count_optimal(orc.agreement(orc.counts(c1), orc.counts(c2)))
        out[f"runs_{tag}_nopt"] = np.int64(nopt)
        assert nopt == 1, (tag, nopt)
    out["runs_planted_in0"], out["runs_planted_in1"] = pack(planted[0]), pack(planted[1])
    out["runs_planted_shape"] = np.array([k2, n2], dtype=np.int64)
    out["runs_planted_relabel"] = np.array(relabel, dtype=np.int8)


def main():
    out = {}
    record_logger(out)
    record_realign(out)
    record_runs(out)
    path = HERE / "align.npz"
    np.savez_compressed(path, **out)
    print(f"[golden-align] wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")
    assert path.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
