"""Cluster labels aligned within a run and across runs, on the device (include/sbe_align.h).

Cluster labels are arbitrary: area 0 of one sample, or of one run, is in general not area 0 of the next, so the indicator
columns `a{k}_{object}`, `size_a{k}` and `areal_a{k}_*` of two converged runs disagree until the labels are matched.  The
reference matches every logged sample against the running sum of the samples aligned so far (its loggers), re-aligns a
finished run from a seed of 20 samples (tools/realign_clusters_within_run.py) and matches two runs by their mean
memberships (tools/align_clusters.py).  This module does the three on the GPU:

    perms = match_online(clusters)                        # clusters: 0/1 [S, K, N]; the loggers' rule (seed 0)
    perms = realign_within_run(clusters, seed=20)         # the tool's rule, in the raw frame
    res = align_runs([run0, run1, run2], pivot=0, within=20, burnin=0.1)
    aligned = apply(run1, res.total_perms[1]); names, rows = permute_stats(names, rows, res.total_perms[1])
    python -m sbayes_amd.align -k 3 results_dir 0 1 2 --within 20 --pivot 0

Contract (tests/_align_oracle.py restates it in NumPy; DESIGN.md section 17 states it).  For an integer agreement matrix
d[K][K] the permutation p maximises sum_i d[i][p[i]]; among the maximisers it is the lexicographically smallest sequence
(p[0], ..., p[K-1]).  The aligned sample is c[p] (label i takes cluster p[i]).  Wherever the optimum is unique this is the
reference's scipy.optimize.linear_sum_assignment(d, maximize=True)[1]; under ties SciPy's choice is not reproduced.
Within a run with seed m0: m = min(m0, S), w = max(m, 1), sum = the raw first m samples added up; for every sample s in
order, d = sum @ c[s].T, P_s = rule(d), sum += w * c[s][P_s].  Counts: cnt[r][i][n] = sum over s >= burn_r of
c[s][P_s[i]][n].  Across runs with pivot a: d = cnt[a] @ cnt[b].T, Q_b = rule(d).  All of it in exact integers.
Limits: 1 <= K <= 8; N <= max_objects(K) (the running sums live in LDS); at most 64 runs of at most 2^20 samples;
seed <= 1024.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _clusters, _handle, diag
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_ALIGN_ABI_VERSION of include/sbe_align.h
MAX_CLUSTERS = 8                         # SBE_ALIGN_MAX_CLUSTERS
MAX_RUNS = 64                            # SBE_ALIGN_MAX_RUNS
MAX_ROWS = 1 << 20                       # SBE_ALIGN_MAX_ROWS
MAX_SEED_ROWS = 1024                     # SBE_ALIGN_MAX_SEED_ROWS
LDS_BYTES = 160 * 1024                   # SBE_ALIGN_LDS_BYTES
STATIC_LDS = 4096                        # SBE_ALIGN_STATIC_LDS

# name -> (restype, argtypes); mirrors include/sbe_align.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.store_prototypes("sbe_align", [ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_align_max_objects": (ct.c_int64, [ct.c_int]),
    "sbe_align_within": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p]),
    "sbe_align_counts": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p, ct.c_void_p]),
    "sbe_align_runs": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_align.h attached."""
    return _handle.bind("sbe_align", PROTOTYPES, ABI_VERSION)


def max_objects(n_clusters) -> int:
    """Largest N for K clusters: the int32 running sums [K][N] and the kernel's own LDS fit the 160 KiB of a CU."""
    n_clusters = int(n_clusters)
    if not 1 <= n_clusters <= MAX_CLUSTERS:
        raise ValueError(f"{n_clusters} clusters; the alignment takes 1 .. {MAX_CLUSTERS}")
    return (LDS_BYTES - STATIC_LDS) // (4 * n_clusters)


# ---- validation (host side, before any library call) -----------------------------------------------------------
LIMITS = _clusters.StoreLimits("the alignment", MAX_CLUSTERS, max_objects, MAX_ROWS, "(the running sums live in LDS)", max_runs=MAX_RUNS)


def _check_seed(seed):
    seed = int(seed)
    if not 0 <= seed <= MAX_SEED_ROWS:
        raise ValueError(f"seed={seed} must lie in [0, {MAX_SEED_ROWS}]")
    return seed


def _check_runs(runs):
    blocks, k, n = _clusters.check_runs(LIMITS, runs)
    LIMITS.check_shape(*_clusters.store_shape(blocks, k, n))
    return blocks, k, n


class AlignHandle(_clusters.SampleStoreHandle):
    """Owner of one sbe_align handle: the bit store of several runs of cluster samples on one device.
    last_kernel_ms(): the within-run kernel of the last within() call."""
    _prefix, _noun, _limits = "sbe_align", "an alignment handle", LIMITS

    def append(self, run, clusters):
        """Append samples ([n, K, N] of 0 / 1, or one sample [K, N]) to a run.  (The store has no operand image: a failed
        append leaves its shape.)"""
        run, block = self._checked_block(run, clusters)
        self._check(self._append_rows(run, block))
        self._stored[run] += block.shape[0]

    def within(self, seed=0):
        """One permutation per stored sample of every run: a list of int8 [S_r, K] arrays."""
        self._shaped()
        seed = _check_seed(seed)
        perms = np.zeros((self.n_runs, self.capacity, self.n_clusters), dtype=np.int8)
        self._check(self._lib.sbe_align_within(self._h, seed, _ptr(perms)))
        return [perms[r, :self.rows(r)].copy() for r in range(self.n_runs)]

    def _burn(self, burn_rows):
        self._shaped()
        burn = np.zeros(self.n_runs, dtype=np.int64) if burn_rows is None else np.ascontiguousarray(burn_rows, dtype=np.int64)
        if burn.shape != (self.n_runs,):
            raise ValueError(f"burn_rows must hold one value per run ({self.n_runs}), got shape {burn.shape}")
        return burn

    def counts(self, aligned=True, burn_rows=None):
        """Membership counts int32 [R, K, N] over the samples from burn_rows[r] on, through the permutations of the last
        within() (aligned=True) or as stored."""
        burn = self._burn(burn_rows)
        counts = np.empty((self.n_runs, self.n_clusters, self.n_objects), dtype=np.int32)
        self._check(self._lib.sbe_align_counts(self._h, int(bool(aligned)), _ptr(burn), _ptr(counts)))
        return counts

    def runs(self, pivot=0, aligned=True, burn_rows=None):
        """(run permutations int8 [R, K], agreement matrices int64 [R, K, K]) of every run against run `pivot`."""
        burn = self._burn(burn_rows)
        pivot = self._check_lane(pivot)
        run_perms = np.empty((self.n_runs, self.n_clusters), dtype=np.int8)
        agreement = np.empty((self.n_runs, self.n_clusters, self.n_clusters), dtype=np.int64)
        self._check(self._lib.sbe_align_runs(self._h, pivot, int(bool(aligned)), _ptr(burn), _ptr(run_perms), _ptr(agreement)))
        return run_perms, agreement


@dataclass
class AlignResult:
    """perms[r]: int8 [S_r, K], the within-run permutation of every sample (the identity without within-run alignment);
    run_perms: int8 [R, K]; total_perms[r][s] = perms[r][s][run_perms[r]], what apply() and permute_stats() take to bring
    run r's sample s into the pivot's labels; counts int32 and frequencies float64 [R, K, N] in the pivot's labels, over
    the samples after burn-in; agreement: int64 [R, K, K], the matrices the run permutations were chosen on (rows: the
    pivot's labels, columns: the run's own labels after within-run alignment); burn_rows per run."""
    perms: list
    run_perms: np.ndarray
    total_perms: list
    counts: np.ndarray
    frequencies: np.ndarray
    agreement: np.ndarray
    burn_rows: tuple
    pivot: int = 0
    kernel_ms: float = 0.0

    def agreement_before(self, r) -> int:
        """The agreement of run r with the pivot under the labels it came with (the trace of its matrix)."""
        return int(np.trace(self.agreement[r]))

    def agreement_after(self, r) -> int:
        k = self.agreement.shape[1]
        return int(self.agreement[r][np.arange(k), self.run_perms[r]].sum())


def _within(blocks, k, n, seed, device):
    h = AlignHandle.filled(device, _clusters.store_shape(blocks, k, n), blocks)
    try:
        return h.within(seed)
    finally:
        h.close()


def realign_within_run(clusters, seed=20, device=None):
    """int8 [S, K]: the permutation of every sample of one run against the seed (the first `seed` samples added up) plus
    the aligned samples before it; seed=20 is realign_clusters_within_run.align_clusters, in the raw frame."""
    seed = _check_seed(seed)
    blocks, k, n = _check_runs([clusters])
    return _within(blocks, k, n, seed, device)[0]


def match_online(clusters, device=None):
    """int8 [S, K]: the permutation the reference's loggers apply to every sample of one run as it is logged."""
    return realign_within_run(clusters, seed=0, device=device)


def align_runs(runs, pivot=0, within=None, burnin=0.0, device=None) -> AlignResult:
    """Align the labels of several runs (a list of 0/1 [S_r, K, N] arrays) to those of run `pivot`.  within: None takes
    every run as logged, 0 or 20 first aligns the samples of each run with that seed.  burnin: the share of each run's
    samples left out of the membership counts the runs are matched on."""
    blocks, k, n = _check_runs(runs)
    pivot = int(pivot)
    if not 0 <= pivot < len(blocks):
        raise ValueError(f"pivot {pivot} out of range [0, {len(blocks)})")
    seed = None if within is None else _check_seed(within)
    burn = _clusters.burn_rows([b.shape[0] for b in blocks], burnin)
    h = AlignHandle.filled(device, _clusters.store_shape(blocks, k, n), blocks)
    try:
        if seed is None:
            perms = [np.tile(np.arange(k, dtype=np.int8), (b.shape[0], 1)) for b in blocks]
            kernel_ms = 0.0
        else:
            perms = h.within(seed)
            kernel_ms = h.last_kernel_ms()
        counts = h.counts(aligned=seed is not None, burn_rows=burn)
        run_perms, agreement = h.runs(pivot, aligned=seed is not None, burn_rows=burn)
    finally:
        h.close()
    counts = np.stack([counts[r][run_perms[r]] for r in range(len(blocks))])
    kept = np.array([max(b.shape[0] - br, 1) for b, br in zip(blocks, burn)], dtype=np.float64)
    total = [p[:, q] for p, q in zip(perms, run_perms)]
    return AlignResult(perms, run_perms, total, counts, counts / kept[:, None, None], agreement, tuple(burn), pivot, kernel_ms)


# ---- host-side application ---------------------------------------------------------------------------------------
def _check_perms(perms, s, k):
    p = np.asarray(perms)
    if p.ndim == 1:
        p = np.broadcast_to(p, (s, p.shape[0]))
    if p.shape != (s, k):
        raise ValueError(f"permutations must be [{s}, {k}] (or one of [{k}]), got shape {p.shape}")
    if not np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(k), (s, k))):
        raise ValueError("a row is not a permutation of the cluster labels")
    return p.astype(np.intp)


def apply(clusters, perms):
    """The aligned samples: out[s][i] = clusters[s][perms[s][i]] (perms: [S, K], or one permutation [K] for all)."""
    c = np.asarray(clusters)
    if c.ndim != 3:
        raise ValueError(f"cluster samples must be [n_samples, n_clusters, n_objects], got shape {c.shape}")
    p = _check_perms(perms, c.shape[0], c.shape[1])
    return np.take_along_axis(c, p[:, :, None], axis=1)


_CLUSTER_COLUMN = re.compile(r"^(size|post|lh|prior)_a(\d+)$|^areal_a(\d+)_(.*)$")


def permute_stats(names, rows, perms):
    """The rows of a stats table with the per-cluster columns moved as the cluster labels move: row s of `size_a{i}`,
    `areal_a{i}_*` and, where present, `post_a{i}`, `lh_a{i}`, `prior_a{i}` takes the value the row has at label
    perms[s][i].  A true permutation of the columns row by row; every other column stays.  Returns (names, new rows)."""
    names = [str(v) for v in names]
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != len(names):
        raise ValueError(f"rows must be [n_samples, {len(names)}], got shape {rows.shape}")
    groups = {}                                                             # (kind, rest) -> {label: column}
    for col, name in enumerate(names):
        m = _CLUSTER_COLUMN.match(name)
        if m:
            key = (m.group(1), "") if m.group(1) else ("areal", m.group(4))
            groups.setdefault(key, {})[int(m.group(2) if m.group(1) else m.group(3))] = col
    if not groups:
        return names, rows.copy()
    k = 1 + max(max(g) for g in groups.values())
    p = _check_perms(perms, rows.shape[0], k)
    out = rows.copy()
    for key, cols in groups.items():
        if sorted(cols) != list(range(k)):
            raise ValueError(f"the columns {key[0]}_a*{'_' + key[1] if key[1] else ''} do not cover the labels 0 .. {k - 1}")
        index = np.array([cols[i] for i in range(k)])
        out[:, index] = np.take_along_axis(rows[:, index], p, axis=1)
    return names, out


# ---- the reference's files ------------------------------------------------------------------------------------
def read_clusters(path):
    """uint8 [S, K, N] of a clusters file: one line per sample of K tab-separated strings of N characters 0 / 1."""
    names, rows = diag.read_clusters(path)
    k = 1 + int(names[-1].split("_")[0][1:])
    return rows.astype(np.uint8).reshape(rows.shape[0], k, rows.shape[1] // k)


def write_clusters(path, clusters):
    """Write samples [S, K, N] in the ClustersLogger format."""
    c = _clusters.check_samples(clusters)
    table = np.array([ord("0"), ord("1")], dtype=np.uint8)[c]
    with open(path, "w") as f:
        for sample in table:
            f.write("\t".join(row.tobytes().decode("ascii") for row in sample) + "\n")


def read_stats_text(path):
    """(header names, rows as lists of strings) of a stats file: every column, as the text holds it."""
    with open(path, "r") as f:
        header = f.readline().rstrip("\n").split("\t")
        cells = [line.rstrip("\n").split("\t") for line in f if line.strip()]
    if any(len(c) != len(header) for c in cells):
        raise ValueError(f"{path}: a line does not have the header's {len(header)} columns")
    return header, cells


def write_stats_text(path, header, cells):
    with open(path, "w") as f:
        f.write("\t".join(header) + "\n")
        for row in cells:
            f.write("\t".join(row) + "\n")


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sbayes_amd.align",
                                 description="Align the cluster labels of several sBayes runs, within each run and across them")
    ap.add_argument("-k", type=int, required=True, help="number of clusters: the files are <results_dir>/K<k>/clusters_K<k>_<run>.txt")
    ap.add_argument("results_dir", type=Path)
    ap.add_argument("runs", nargs="+", help="run names, as in the file names")
    ap.add_argument("--within", type=int, choices=[0, 20], default=None, help="first align the samples of each run (seed 0 or 20)")
    ap.add_argument("--pivot", default=None, help="the run whose labels the others take (default: the first)")
    ap.add_argument("--burnin", type=float, default=0.0)
    ap.add_argument("--device", type=int, default=None)
    args = ap.parse_args(argv)
    k = args.k
    folder = args.results_dir / f"K{k}"
    if not folder.is_dir():
        folder = args.results_dir
    pivot_name = args.runs[0] if args.pivot is None else args.pivot
    if pivot_name not in args.runs:
        raise SystemExit(f"pivot {pivot_name} is not among the runs {args.runs}")
    pivot = args.runs.index(pivot_name)
    runs = [read_clusters(folder / f"clusters_K{k}_{run}.txt") for run in args.runs]
    if any(c.shape[1] != k for c in runs):
        raise SystemExit(f"a clusters file does not hold {k} clusters per sample")
    res = align_runs(runs, pivot=pivot, within=args.within, burnin=args.burnin, device=args.device)
    print(f"{len(runs)} runs, {k} clusters, {runs[0].shape[2]} objects; pivot {pivot_name}; within-run alignment: "
          f"{'none' if args.within is None else 'seed %d' % args.within} (kernel {res.kernel_ms:.3f} ms)")
    for r, run in enumerate(args.runs):
        moved = int(np.count_nonzero((res.perms[r] != np.arange(k)).any(axis=1)))
        print(f"run {run}: permutation {res.run_perms[r].tolist()}  agreement with the pivot {res.agreement_before(r)} -> "
              f"{res.agreement_after(r)}  ({moved} of {runs[r].shape[0]} samples moved within the run)")
        write_clusters(folder / f"clusters_K{k}_{run}.aligned.txt", apply(runs[r], res.total_perms[r]))
        stats_path = folder / f"stats_K{k}_{run}.txt"
        if stats_path.exists():
            header, cells = read_stats_text(stats_path)
            if len(cells) != runs[r].shape[0]:
                raise SystemExit(f"run {run}: {len(cells)} stats rows, {runs[r].shape[0]} cluster samples")
            _names, moved_cells = permute_stats(header, np.array(cells, dtype=object).reshape(len(cells), len(header)), res.total_perms[r])
            write_stats_text(folder / f"stats_K{k}_{run}.aligned.txt", header, [list(map(str, row)) for row in moved_cells])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
