"""Posterior similarity of objects and a consensus clustering, on the device (include/sbe_consensus.h).

align, diag and summary look at a clustering through its labels.  This module is label free: it counts how often two
objects share an area over the cluster samples of one or several runs (the posterior similarity, or co-clustering,
matrix) and reads three things from it: how often two objects go together, whether two runs agree -- with no label
matching at all -- and which logged sample is the consensus (Dahl's least-squares clustering: the sample that minimises
Binder's loss against the matrix).  The reference has no tool for this.

    sim = similarity([run0, run1], burnin=0.1)            # runs: 0/1 [S_r, K, N]; sim.counts, sim.n_samples, sim.probability
    est = point_estimate([run0, run1], burnin=0.1)        # est.run, est.sample, est.clusters [K, N], est.scores
    cmp = compare_runs([run0, run1, run2])                # cmp.max_abs, cmp.mean_abs: float64 [R, R]
    python -m sbayes_amd.consensus clusters_K3_*.txt --burnin 0.1 --out DIR

Contract (tests/_consensus_oracle.py restates it in NumPy; DESIGN.md section 19 states it), all in exact integers.  For a
selection of runs with T samples in all: counts C[i][j] = the number of (sample, cluster) rows that hold both i and j,
int32 [N, N]; with disjoint areas C / T is the posterior probability that i and j share an area.  The score of a sample
against (C, T) is sum_k sum_{i,j in cluster k} (T - 2 C[i][j]), int64; for disjoint areas T^2 Binder = T score + sum C^2,
so the smallest score is the least-squares sample, and the consensus is the sample with the smallest (score, run, sample).
Two matrices (C_a, T_a), (C_b, T_b) are compared through d = |C_a T_b - C_b T_a|: its row maxima and row sums come from
the device, max |P_a - P_b| and mean |P_a - P_b| are formed here with Python integers over T_a T_b.
Limits: 1 <= K <= 8; N <= 16384; at most 64 runs of at most 2^20 samples; T K <= 2^24 for a selection (the matrix pipe's
f32 accumulator is exact up to there); a store of at most 16 GiB on the device (image_bytes).

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _clusters, _handle, align
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_CONSENSUS_ABI_VERSION of include/sbe_consensus.h
MAX_CLUSTERS = 8                         # SBE_CONSENSUS_MAX_CLUSTERS
MAX_OBJECTS = 16384                      # SBE_CONSENSUS_MAX_OBJECTS
MAX_RUNS = 64                            # SBE_CONSENSUS_MAX_RUNS
MAX_ROWS = 1 << 20                       # SBE_CONSENSUS_MAX_ROWS
MAX_ELEMENTS = 1 << 24                   # SBE_CONSENSUS_MAX_ELEMENTS
ROUND = 256                              # SBE_CONSENSUS_ROUND
MAX_IMAGE_BYTES = 1 << 34                # SBE_CONSENSUS_MAX_IMAGE_BYTES

# name -> (restype, argtypes); mirrors include/sbe_consensus.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.store_prototypes("sbe_consensus", [ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_consensus_image_bytes": (ct.c_int64, [ct.c_int, ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_consensus_similarity": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_void_p]),
    "sbe_consensus_scores": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int, ct.c_void_p]),
    "sbe_consensus_compare": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p]),
    "sbe_consensus_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
}


def load():
    """The engine library with the prototypes of include/sbe_consensus.h attached."""
    return _handle.bind("sbe_consensus", PROTOTYPES, ABI_VERSION)


def image_bytes(n_runs, n_clusters, n_objects, capacity) -> int:
    """Device bytes of a store of this shape: the FP4 operand image (whole tiles of 32 objects, one segment per run padded
    to whole rounds of 256 elements, a nibble per element) plus the bit rows."""
    words = (int(n_objects) + 31) // 32
    segment = (int(capacity) * int(n_clusters) + ROUND - 1) // ROUND * (ROUND // 2)
    return 32 * words * int(n_runs) * segment + int(n_runs) * int(capacity) * int(n_clusters) * words * 4


# ---- validation (host side, before any library call) -----------------------------------------------------------
LIMITS = _clusters.StoreLimits("the consensus store", MAX_CLUSTERS, MAX_OBJECTS, MAX_ROWS, "(an int32 matrix [N, N] of at most 1 GiB)",
                               max_runs=MAX_RUNS, image_bytes=image_bytes, max_image_bytes=MAX_IMAGE_BYTES)


def _check_elements(n_samples, n_clusters):
    if n_samples < 1:
        raise ValueError("the selected runs hold no samples")
    if n_samples * n_clusters > MAX_ELEMENTS:
        raise ValueError(f"the selection holds {n_samples} samples x {n_clusters} clusters = {n_samples * n_clusters} elements, the limit is "
                         f"{MAX_ELEMENTS} (2^24: the counts are exact in the f32 accumulator up to there)")


def _check_runs(runs, burnin):
    """The runs after burn-in (uint8 [S_r, K, N], C order), K, N."""
    blocks, k, n = _clusters.check_runs(LIMITS, runs)
    LIMITS.check_shape(*_clusters.store_shape(blocks, k, n))
    return _clusters.after_burnin(blocks, burnin), k, n


class ConsensusHandle(_clusters.SampleStoreHandle):
    """Owner of one sbe_consensus handle: the store of several runs of cluster samples on one device and two similarity
    matrices (slots 0 and 1; both are out of date after an append).  last_kernel_ms(): the kernels of the last similarity(),
    scores() or compare()."""
    _prefix, _noun, _limits = "sbe_consensus", "a consensus handle", LIMITS

    def _out_of_date(self):
        self.slot_samples = [0, 0]                  # T of the matrix in each slot (0: empty or out of date)

    def similarity(self, runs=None, slot=0, copy=True):
        """The similarity counts over `runs` (indices; None: every run) into `slot`; int32 [N, N], or None with copy=False
        (the matrix stays on the device for scores() and compare())."""
        self._shaped()
        slot = _clusters.check_index("slot", slot)
        mask = self._mask(runs)
        total = sum(s for s, m in zip(self._stored, mask) if m)
        _check_elements(total, self.n_clusters)
        counts = np.empty((self.n_objects, self.n_objects), dtype=np.int32) if copy else None
        self.slot_samples[slot] = 0
        self._check(self._lib.sbe_consensus_similarity(self._h, _ptr(mask), slot, _ptr(counts) if copy else None))
        self.slot_samples[slot] = total
        return counts

    def scores(self, run, slot=0):
        """int64 [rows(run)]: the score of every stored sample of `run` against the matrix in `slot`."""
        run, slot = self._check_lane(run), _clusters.check_index("slot", slot)
        scores = np.empty(self._stored[run], dtype=np.int64)
        self._check(self._lib.sbe_consensus_scores(self._h, slot, run, _ptr(scores)))
        return scores

    def compare(self):
        """(row_max, row_sum) int64 [N] of |C_0 T_1 - C_1 T_0|, slot 0 against slot 1."""
        self._shaped()
        row_max = np.empty(self.n_objects, dtype=np.int64)
        row_sum = np.empty(self.n_objects, dtype=np.int64)
        self._check(self._lib.sbe_consensus_compare(self._h, _ptr(row_max), _ptr(row_sum)))
        return row_max, row_sum


@dataclass
class Similarity:
    """counts: int32 [N, N]; n_samples: T, the samples counted; probability = counts / T, float64."""
    counts: np.ndarray
    n_samples: int
    kernel_ms: float = 0.0

    @property
    def probability(self):
        return self.counts / float(self.n_samples)


@dataclass
class PointEstimate:
    """The pooled matrix's least-squares sample: run and sample (counted after burn-in), its clusters uint8 [K, N]; scores:
    one int64 array per run (after burn-in); n_samples: T of the pooled matrix."""
    run: int
    sample: int
    clusters: np.ndarray
    scores: list
    n_samples: int
    kernel_ms: float = 0.0


@dataclass
class RunComparison:
    """max_abs, mean_abs: float64 [R, R], max and mean over the object pairs of |P_a - P_b|, P_r the similarity
    probabilities of run r alone; symmetric, zero on the diagonal.  n_samples: T per run."""
    max_abs: np.ndarray
    mean_abs: np.ndarray
    n_samples: tuple


def _filled(blocks, k, n, device):
    return ConsensusHandle.filled(device, _clusters.store_shape(blocks, k, n), blocks)


def similarity(runs, burnin=0.0, device=None) -> Similarity:
    """The similarity of the objects over all samples of `runs` (a list of 0/1 [S_r, K, N] arrays) after burn-in."""
    blocks, k, n = _check_runs(runs, burnin)
    _check_elements(sum(b.shape[0] for b in blocks), k)
    h = _filled(blocks, k, n, device)
    try:
        counts = h.similarity()
        return Similarity(counts, h.slot_samples[0], h.last_kernel_ms())
    finally:
        h.close()


argmin_score = _clusters.argmin_rows      # (run, sample) of the smallest (score, run, sample) over per-run score arrays


def _estimate(h, blocks, copy=False, clock=lambda: 0.0):
    """point_estimate on a filled handle, and the pooled counts (None without copy).  clock: the handle's last_kernel_ms
    where the caller wants the kernels' time."""
    counts = h.similarity(copy=copy)
    kernel_ms = clock()
    scores = []
    for r in range(len(blocks)):
        scores.append(h.scores(r))
        kernel_ms += clock()
    run, sample = argmin_score(scores)
    return PointEstimate(run, sample, blocks[run][sample].copy(), scores, h.slot_samples[0], kernel_ms), counts


def point_estimate(runs, burnin=0.0, device=None) -> PointEstimate:
    """The consensus clustering: the sample of `runs` (after burn-in) with the smallest score against the pooled matrix."""
    blocks, k, n = _check_runs(runs, burnin)
    _check_elements(sum(b.shape[0] for b in blocks), k)
    h = _filled(blocks, k, n, device)
    try:
        return _estimate(h, blocks, clock=h.last_kernel_ms)[0]
    finally:
        h.close()


def difference(row_max, row_sum, n_a, n_b):
    """(max, mean) of |P_a - P_b| from the row maxima and row sums of |C_a T_b - C_b T_a|: Python integers, one division each."""
    n = len(row_max)
    return int(max(int(v) for v in row_max)) / (n_a * n_b), sum(int(v) for v in row_sum) / (n_a * n_b * n * n)


def _compare(h, lengths) -> RunComparison:
    """compare_runs on a filled handle: every run's own matrix (slot 0) against every later run's (slot 1)."""
    r_n = len(lengths)
    max_abs, mean_abs = np.zeros((r_n, r_n)), np.zeros((r_n, r_n))
    for a in range(r_n - 1):
        h.similarity([a], slot=0, copy=False)
        for b in range(a + 1, r_n):
            h.similarity([b], slot=1, copy=False)
            row_max, row_sum = h.compare()
            max_abs[a, b], mean_abs[a, b] = difference(row_max, row_sum, lengths[a], lengths[b])
            max_abs[b, a], mean_abs[b, a] = max_abs[a, b], mean_abs[a, b]
    return RunComparison(max_abs, mean_abs, tuple(lengths))


def compare_runs(runs, burnin=0.0, device=None) -> RunComparison:
    """Every run's own similarity probabilities against every other run's, with no label matching."""
    blocks, k, n = _check_runs(runs, burnin)
    for b in blocks:
        _check_elements(b.shape[0], k)
    h = _filled(blocks, k, n, device)
    try:
        return _compare(h, [b.shape[0] for b in blocks])
    finally:
        h.close()


# ---- files -------------------------------------------------------------------------------------------------------
def write_similarity(path, probability):
    """The similarity probabilities as a tab-separated table [N, N] (repr of float64: reads back bit for bit)."""
    with open(path, "w") as f:
        for row in np.asarray(probability, dtype=np.float64):
            f.write("\t".join(repr(float(v)) for v in row) + "\n")


def read_similarity(path):
    with open(path, "r") as f:
        return np.array([[float(v) for v in line.split("\t")] for line in f if line.strip()], dtype=np.float64)


def main(argv=None):
    ap = _clusters.runs_parser("python -m sbayes_amd.consensus", "Posterior similarity of the objects, agreement of the runs and the consensus "
                                                                 "clustering of several sBayes runs")
    args = ap.parse_args(argv)
    runs, tag, _names, out = _clusters.read_runs(args)
    blocks, k, n = _check_runs(runs, args.burnin)
    lengths = [b.shape[0] for b in blocks]
    _check_elements(sum(lengths), k)
    h = _filled(blocks, k, n, args.device)                  # one store serves the three questions
    try:
        est, counts = _estimate(h, blocks, copy=True)       # the pooled matrix, slot 0
        cmp = _compare(h, lengths)
    finally:
        h.close()
    r_n = len(blocks)
    print(f"{r_n} runs, {k} clusters, {n} objects; {est.n_samples} samples after burn-in")
    print(f"consensus: sample {est.sample} (after burn-in) of {args.files[est.run].name}, score {int(est.scores[est.run][est.sample])}")
    align.write_clusters(out / f"consensus_{tag}.txt", est.clusters[None])
    write_similarity(out / f"similarity_{tag}.txt", counts / float(est.n_samples))
    if r_n > 1:
        print("max |P_a - P_b| (above the diagonal) and mean |P_a - P_b| (below it) of the runs' similarity probabilities:")
        for a in range(r_n):
            cells = ["-" if a == b else "%.6f" % (cmp.max_abs[a, b] if a < b else cmp.mean_abs[a, b]) for b in range(r_n)]
            print(f"{args.files[a].name}\t" + "\t".join(cells))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
