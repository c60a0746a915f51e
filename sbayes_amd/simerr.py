"""Monte-Carlo error of the posterior similarity matrix, and run agreement measured in it (include/sbe_simerr.h).

consensus.compare_runs says that two runs' co-clustering probabilities differ by max |P_a - P_b| = 0.08, say; this module
says whether 0.08 is sampler noise.  Every run is cut into batches of b consecutive samples, the co-clustering of every
pair of objects is counted per batch on the matrix pipe, and the spread of the batch counts gives the standard error of
every entry of the similarity matrix (batch means).  Two runs are then compared pair of objects by pair of objects through
z^2 = (P_a - P_b)^2 / (se_a^2 + se_b^2), with no label matching at all.

    err = similarity_error([run0, run1], burnin=0.1)      # runs: 0/1 [S_r, K, N]; err.probability, err.se, err.ess: [N, N]
    agr = run_agreement([run0, run1, run2])               # agr.max_z2 [R, R], agr.pair [R, R, 2], agr.share [R, R, M], ...
    python -m sbayes_amd.simerr clusters_K3_*.txt --burnin 0.1 [--batch N] --out DIR

What the numbers are NOT.  With nB batches per side, z^2 is closer to a squared t statistic (about nB - 1 degrees of freedom,
fewer when the two sides' errors differ) than to chi-squared with one degree of freedom: with few batches 3.84 is passed far
more often than one time in twenty.  The pairs of objects are dependent (one object that moves changes a whole row), so the
shares of pairs above a threshold describe a comparison; they do not test anything.  Batches shorter than the chain's
autocorrelation time make se too small and z^2 too large.  The default batch length, floor(sqrt(S)) of the shortest run, is
the usual compromise between few long batches and many short ones and is not tuned to the chains.

Contract (tests/_simerr_oracle.py restates it in NumPy; DESIGN.md section 30 states it), integers exact.  Batch q of a run is
its samples [q b, (q + 1) b); a trailing incomplete batch is not used.  For a side (a selection of runs) with nB complete
batches: c_q[i][j] = the (sample, cluster) rows of batch q that hold both i and j; S1 = sum_q c_q (int32), S2 = sum_q c_q^2
(int64), V = nB S2 - S1^2 >= 0; P = S1 / (nB b), se^2 = V / (nB^2 (nB - 1) b^2).  When b divides every run's length S1 is
consensus.similarity's counts.  For side a against side b, D = S1_a nB_b - S1_b nB_a and
z^2 = D^2 / (nB_b^2 V_a / (nB_a - 1) + nB_a^2 V_b / (nB_b - 1)) in float64 in the order the header states; 0 where D = 0 and
both V are 0, +inf where only D is not.  Per row: the maximum, the smallest column that attains it, and the number of columns
strictly above each of up to four thresholds.
Limits: 1 <= K <= 8; N <= 8192; at most 64 runs of at most 2^20 samples; 1 <= b <= capacity; nB b K <= 2^24 for a side (the
matrix pipe's f32 accumulator is exact up to there); a side needs two batches; an image of at most 16 GiB (image_bytes).

The one-call functions drop the burn-in and then each run's leading S_r mod b samples, so the most recent samples are all
used.  There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process
model (sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import math
from dataclasses import dataclass

import numpy as np

from . import _clusters, _handle, consensus
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_SIMERR_ABI_VERSION of include/sbe_simerr.h
MAX_CLUSTERS = 8                         # SBE_SIMERR_MAX_CLUSTERS
MAX_OBJECTS = 8192                       # SBE_SIMERR_MAX_OBJECTS
MAX_RUNS = 64                            # SBE_SIMERR_MAX_RUNS
MAX_ROWS = 1 << 20                       # SBE_SIMERR_MAX_ROWS
MAX_ELEMENTS = 1 << 24                   # SBE_SIMERR_MAX_ELEMENTS
STEP = 64                                # SBE_SIMERR_STEP
MAX_THRESHOLDS = 4                       # SBE_SIMERR_MAX_THRESHOLDS
MAX_IMAGE_BYTES = 1 << 34                # SBE_SIMERR_MAX_IMAGE_BYTES
THRESHOLDS = (3.84, 6.63, 10.83)         # the 0.05, 0.01 and 0.001 points of chi-squared with one degree of freedom

# name -> (restype, argtypes); mirrors include/sbe_simerr.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.store_prototypes("sbe_simerr", [ct.c_int, ct.c_int64, ct.c_int64, ct.c_int64]),
    "sbe_simerr_image_bytes": (ct.c_int64, [ct.c_int, ct.c_int, ct.c_int64, ct.c_int64, ct.c_int64]),
    "sbe_simerr_moments": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_int64)]),
    "sbe_simerr_compare": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_simerr_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
}


def load():
    """The engine library with the prototypes of include/sbe_simerr.h attached."""
    return _handle.bind("sbe_simerr", PROTOTYPES, ABI_VERSION)


def image_bytes(n_runs, n_clusters, n_objects, capacity, batch_rows) -> int:
    """Device bytes of a store of this shape: the FP4 operand image (whole tiles of 32 objects, one segment per run, every
    batch padded to whole steps of 64 elements, a nibble per element)."""
    batches = -(-int(capacity) // int(batch_rows))
    steps = -(-int(batch_rows) * int(n_clusters) // STEP)
    return 32 * ((int(n_objects) + 31) // 32) * int(n_runs) * batches * steps * (STEP // 2)


# ---- validation (host side, before any library call) -----------------------------------------------------------
LIMITS = _clusters.StoreLimits("the similarity-error store", MAX_CLUSTERS, MAX_OBJECTS, MAX_ROWS, "(a side holds 12 N^2 bytes: at most 768 MiB)",
                               max_runs=MAX_RUNS, image_bytes=image_bytes, max_image_bytes=MAX_IMAGE_BYTES)


def _check_shape(n_runs, n_clusters, n_objects, capacity, batch_rows):
    LIMITS.check_ranges(n_runs, n_clusters, n_objects, capacity)
    if not 1 <= batch_rows <= capacity:
        raise ValueError(f"batch_rows={batch_rows} out of range [1, {capacity}] (the capacity of a run)")
    LIMITS.check_image(n_runs, n_clusters, n_objects, capacity, batch_rows, how=f" in batches of {batch_rows}")


def _check_side_batches(n_batches, batch_rows, n_samples, n_clusters):
    """A side of n_batches complete batches of batch_rows samples, cut from n_samples stored ones."""
    if n_batches < 2:
        raise ValueError(f"the selected runs hold {n_batches} complete batches of {batch_rows} samples ({n_samples} samples in all); "
                         "a side takes at least 2 batches")
    used = n_batches * batch_rows
    if used * n_clusters > MAX_ELEMENTS:
        raise ValueError(f"the side holds {used} samples x {n_clusters} clusters = {used * n_clusters} elements, the limit is "
                         f"{MAX_ELEMENTS} (2^24: the counts are exact in the f32 accumulator up to there)")


def _check_thresholds(thresholds):
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1) if len(thresholds) else np.zeros(0, dtype=np.float64)
    if thr.size > MAX_THRESHOLDS:
        raise ValueError(f"{thr.size} thresholds; a comparison takes 0 .. {MAX_THRESHOLDS}")
    if np.isnan(thr).any():
        raise ValueError(f"thresholds={[float(v) for v in thr]} hold a value that is not a number")
    return thr


def default_batch_rows(lengths) -> int:
    """max(1, floor(sqrt(min_r S_r))): the usual compromise, not tuned."""
    return max(1, math.isqrt(max(0, min(int(s) for s in lengths))))


def _check_runs(runs, burnin, batch_rows):
    """The runs after burn-in and without their leading S_r mod b samples (uint8 [nB_r b, K, N], C order), K, N, b.  (The store
    is shaped to what the burn-in leaves, so its shape is checked behind it.)"""
    blocks, k, n = _clusters.check_runs(LIMITS, runs)
    blocks = _clusters.after_burnin(blocks, burnin)
    if batch_rows is None:
        batch_rows = default_batch_rows([b.shape[0] for b in blocks])
    elif isinstance(batch_rows, bool) or int(batch_rows) != batch_rows:
        raise ValueError(f"batch_rows={batch_rows!r} is not a whole number")
    batch_rows = int(batch_rows)
    _check_shape(*_clusters.store_shape(blocks, k, n), batch_rows)
    return [b[b.shape[0] % batch_rows:] for b in blocks], k, n, batch_rows


@dataclass
class Moments:
    """s1: int32 [N, N], s2: int64 [N, N] (None where a call left them on the device); n_batches: nB of the side."""
    s1: np.ndarray
    s2: np.ndarray
    n_batches: int

    @property
    def variance(self):
        """V = nB S2 - S1^2, int64."""
        s1 = self.s1.astype(np.int64)
        return self.n_batches * self.s2 - s1 * s1


@dataclass
class Comparison:
    """z2: float64 [N, N] or None; row_max: float64 [N]; row_arg: int32 [N], the smallest column that attains the maximum;
    row_count: int32 [N, M], columns strictly above each threshold."""
    z2: np.ndarray
    row_max: np.ndarray
    row_arg: np.ndarray
    row_count: np.ndarray


class SimErrHandle(_clusters.SampleStoreHandle):
    """Owner of one sbe_simerr handle: the store of several runs of cluster samples in batches on one device and the
    moments of two sides (0 and 1; both are out of date after an append).  last_kernel_ms(): the kernels of the last moments()
    or compare()."""
    _prefix, _noun, _limits = "sbe_simerr", "a similarity-error handle", LIMITS
    _check_shape = staticmethod(_check_shape)

    def _unshape(self):
        super()._unshape()
        self.batch_rows = 0

    def _out_of_date(self):
        self.side_batches = [0, 0]                  # nB of each side (0: empty or out of date)

    def reset(self, n_runs, n_clusters, n_objects, capacity, batch_rows):
        """Shape the store: n_runs empty runs of up to `capacity` samples of n_clusters x n_objects bits, in batches of
        `batch_rows` samples."""
        super().reset(n_runs, n_clusters, n_objects, capacity, batch_rows)
        self.batch_rows = int(batch_rows)

    def moments(self, runs=None, side=0, copy=True) -> Moments:
        """The moments over the complete batches of `runs` (indices; None: every run) into `side`; with copy=False S1 and S2
        stay on the device for compare() and only n_batches is returned."""
        self._shaped()
        side = _clusters.check_index("side", side)
        mask = self._mask(runs)
        stored = [s for s, m in zip(self._stored, mask) if m]
        _check_side_batches(sum(s // self.batch_rows for s in stored), self.batch_rows, sum(stored), self.n_clusters)
        s1 = np.empty((self.n_objects, self.n_objects), dtype=np.int32) if copy else None
        s2 = np.empty((self.n_objects, self.n_objects), dtype=np.int64) if copy else None
        n_batches = ct.c_int64(0)
        self.side_batches[side] = 0
        self._check(self._lib.sbe_simerr_moments(self._h, _ptr(mask), side, _ptr(s1) if copy else None, _ptr(s2) if copy else None,
                                                 ct.byref(n_batches)))
        self.side_batches[side] = n_batches.value
        return Moments(s1, s2, n_batches.value)

    def compare(self, thresholds=THRESHOLDS, z2=False) -> Comparison:
        """Side 0 against side 1: z^2 of every pair of objects (returned only with z2=True), its row maxima, their columns and
        the columns strictly above each threshold."""
        self._shaped()
        thr = _check_thresholds(thresholds)
        n = self.n_objects
        full = np.empty((n, n), dtype=np.float64) if z2 else None
        row_max = np.empty(n, dtype=np.float64)
        row_arg = np.empty(n, dtype=np.int32)
        row_count = np.empty((n, thr.size), dtype=np.int32)
        self._check(self._lib.sbe_simerr_compare(self._h, _ptr(thr) if thr.size else None, thr.size, _ptr(full) if z2 else None, _ptr(row_max),
                                                 _ptr(row_arg), _ptr(row_count) if thr.size else None))
        return Comparison(full, row_max, row_arg, row_count)


# ---- what the host forms from the integers -------------------------------------------------------------------------------
def standard_error(variance, n_batches, batch_rows):
    """se = sqrt(V / (nB^2 (nB - 1) b^2)), float64."""
    return np.sqrt(np.asarray(variance, dtype=np.int64).astype(np.float64) / float(n_batches * n_batches * (n_batches - 1) * batch_rows * batch_rows))


def z_squared(s1_a, v_a, nb_a, s1_b, v_b, nb_b):
    """z^2 of the header from the integers of two sides, in its float64 order (what the device computes, for entries the host
    holds anyway: the diagonal in run_agreement)."""
    diff = np.asarray(s1_a, dtype=np.int64) * int(nb_b) - np.asarray(s1_b, dtype=np.int64) * int(nb_a)
    d = diff.astype(np.float64)
    num = d * d
    qa = (np.asarray(v_a, dtype=np.int64).astype(np.float64) * float(nb_b * nb_b)) / float(nb_a - 1)
    qb = (np.asarray(v_b, dtype=np.int64).astype(np.float64) * float(nb_a * nb_a)) / float(nb_b - 1)
    den = qa + qb
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, num / den, np.where(diff == 0, 0.0, np.inf))


@dataclass
class SimilarityError:
    """counts: S1, int32 [N, N]; variance: V, int64 [N, N]; n_batches: nB; batch_rows: b; n_samples = nB b, the samples
    used.  probability = counts / n_samples; se: its Monte-Carlo standard error; ess = P (1 - P) / se^2, the number of
    independent samples that would know P as well (inf where se = 0; it reads as a sample size for disjoint areas)."""
    counts: np.ndarray
    variance: np.ndarray
    n_batches: int
    batch_rows: int
    kernel_ms: float = 0.0

    @property
    def n_samples(self):
        return self.n_batches * self.batch_rows

    @property
    def probability(self):
        return self.counts / float(self.n_samples)

    @property
    def se(self):
        return standard_error(self.variance, self.n_batches, self.batch_rows)

    @property
    def ess(self):
        p, se = self.probability, self.se
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(se > 0.0, p * (1.0 - p) / (se * se), np.inf)


@dataclass
class RunAgreement:
    """For every pair of runs (symmetric, the diagonal zero): max_z2 float64 [R, R], the largest z^2 over the pairs of objects;
    pair int32 [R, R, 2], the first pair i <= j that attains it; share float64 [R, R, M], the share of the pairs i <= j with
    z^2 strictly above thresholds[m]; max_abs float64 [R, R], max |P_a - P_b| (consensus.compare_runs' figure on the samples
    used here); object_max float64 [R, R, N], per object the largest z^2 of its row.  n_batches per run; batch_rows: b."""
    max_z2: np.ndarray
    pair: np.ndarray
    share: np.ndarray
    max_abs: np.ndarray
    object_max: np.ndarray
    thresholds: tuple
    n_batches: tuple
    batch_rows: int
    kernel_ms: float = 0.0


def similarity_error(runs, burnin=0.0, batch_rows=None, device=None) -> SimilarityError:
    """The similarity of the objects over `runs` (a list of 0/1 [S_r, K, N] arrays) with its Monte-Carlo standard error by
    batch means.  batch_rows None: floor(sqrt(S)) of the shortest run after burn-in."""
    blocks, k, n, batch_rows = _check_runs(runs, burnin, batch_rows)
    _check_side_batches(sum(b.shape[0] // batch_rows for b in blocks), batch_rows, sum(b.shape[0] for b in blocks), k)
    h = SimErrHandle.filled(device, (*_clusters.store_shape(blocks, k, n), batch_rows), blocks)
    try:
        m = h.moments()
        return SimilarityError(m.s1, m.variance, m.n_batches, batch_rows, h.last_kernel_ms())
    finally:
        h.close()


def _agreement(h, n_runs, thresholds):
    """run_agreement on a filled handle."""
    thr = _check_thresholds(thresholds)
    n, b = h.n_objects, h.batch_rows
    out = RunAgreement(np.zeros((n_runs, n_runs)), np.zeros((n_runs, n_runs, 2), dtype=np.int32), np.zeros((n_runs, n_runs, thr.size)),
                       np.zeros((n_runs, n_runs)), np.zeros((n_runs, n_runs, n)), tuple(float(v) for v in thr), (), b)
    host = {}                                                   # run -> its moments on the host (copied the first time it is computed)
    for a in range(n_runs - 1):
        got = h.moments([a], side=0, copy=a not in host)
        out.kernel_ms += h.last_kernel_ms()
        host.setdefault(a, got)
        for c in range(a + 1, n_runs):
            got = h.moments([c], side=1, copy=c not in host)
            out.kernel_ms += h.last_kernel_ms()
            host.setdefault(c, got)
            cmp = h.compare(thr)
            out.kernel_ms += h.last_kernel_ms()
            ma, mc = host[a], host[c]
            i = int(np.argmax(cmp.row_max))                     # (the first row that attains the maximum; its first column is >= i by symmetry)
            diag = z_squared(np.diag(ma.s1), np.diag(ma.variance), ma.n_batches, np.diag(mc.s1), np.diag(mc.variance), mc.n_batches)
            above = [(int(cmp.row_count[:, m].sum()) + int(np.count_nonzero(diag > thr[m]))) // 2 for m in range(thr.size)]   # (z^2 is symmetric)
            d = np.abs(ma.s1.astype(np.int64) * mc.n_batches - mc.s1.astype(np.int64) * ma.n_batches)
            for p, q in ((a, c), (c, a)):
                out.max_z2[p, q] = cmp.row_max[i]
                out.pair[p, q] = (i, int(cmp.row_arg[i]))
                out.share[p, q] = [v / (n * (n + 1) // 2) for v in above]
                out.max_abs[p, q] = int(d.max()) / (ma.n_batches * mc.n_batches * b)
                out.object_max[p, q] = cmp.row_max
    out.n_batches = tuple(s // b for s in h._stored[:n_runs])
    return out


def run_agreement(runs, burnin=0.0, batch_rows=None, thresholds=THRESHOLDS, device=None) -> RunAgreement:
    """Every run's own similarity probabilities against every other run's, in units of their Monte-Carlo error, with no label
    matching.  Every run needs two complete batches."""
    blocks, k, n, batch_rows = _check_runs(runs, burnin, batch_rows)
    _check_thresholds(thresholds)
    for b in blocks:
        _check_side_batches(b.shape[0] // batch_rows, batch_rows, b.shape[0], k)
    h = SimErrHandle.filled(device, (*_clusters.store_shape(blocks, k, n), batch_rows), blocks)
    try:
        return _agreement(h, len(blocks), thresholds)
    finally:
        h.close()


# ---- files -------------------------------------------------------------------------------------------------------
def write_agreement(path, names, agreement):
    """One line per pair of runs a < b, tab-separated: the runs, their batches, the largest z^2 and its pair of objects,
    max |P_a - P_b| and the share of pairs above each threshold (repr of float64)."""
    with open(path, "w") as f:
        f.write("\t".join(["run_a", "run_b", "batches_a", "batches_b", "batch_rows", "max_z2", "object_i", "object_j", "max_abs"]
                          + [f"share_above_{t!r}" for t in agreement.thresholds]) + "\n")
        for a in range(len(names)):
            for b in range(a + 1, len(names)):
                cells = [names[a], names[b], agreement.n_batches[a], agreement.n_batches[b], agreement.batch_rows, repr(float(agreement.max_z2[a, b])),
                         int(agreement.pair[a, b, 0]), int(agreement.pair[a, b, 1]), repr(float(agreement.max_abs[a, b]))]
                f.write("\t".join(str(c) for c in cells + [repr(float(v)) for v in agreement.share[a, b]]) + "\n")


def main(argv=None):
    ap = _clusters.runs_parser("python -m sbayes_amd.simerr", "Monte-Carlo standard error of the posterior similarity of the objects (batch "
                                                              "means) and the agreement of several sBayes runs in units of it")
    ap.add_argument("--batch", type=int, default=None, help="samples per batch (default: floor(sqrt(S)) of the shortest run after burn-in)")
    args = ap.parse_args(argv)
    runs, tag, _names, out = _clusters.read_runs(args)
    blocks, k, n, batch_rows = _check_runs(runs, args.burnin, args.batch)
    for b in blocks:
        _check_side_batches(b.shape[0] // batch_rows, batch_rows, b.shape[0], k)
    _check_side_batches(sum(b.shape[0] // batch_rows for b in blocks), batch_rows, sum(b.shape[0] for b in blocks), k)
    h = SimErrHandle.filled(args.device, (*_clusters.store_shape(blocks, k, n), batch_rows), blocks)      # one store serves both questions
    try:
        pooled = h.moments()
        agreement = _agreement(h, len(blocks), THRESHOLDS)
    finally:
        h.close()
    err = SimilarityError(pooled.s1, pooled.variance, pooled.n_batches, batch_rows)
    print(f"{len(blocks)} runs, {k} clusters, {n} objects; {err.n_samples} samples in {err.n_batches} batches of {batch_rows} after burn-in")
    print(f"largest standard error of a similarity probability: {float(err.se.max()):.6f}")
    consensus.write_similarity(out / f"similarity_se_{tag}.txt", err.se)
    write_agreement(out / f"agreement_{tag}.tsv", [p.name for p in args.files], agreement)
    for a in range(len(blocks)):
        for b in range(a + 1, len(blocks)):
            print(f"{args.files[a].name} against {args.files[b].name}: max z^2 {agreement.max_z2[a, b]:.3f} at objects "
                  f"{tuple(int(v) for v in agreement.pair[a, b])}, max |P_a - P_b| {agreement.max_abs[a, b]:.6f}, share of pairs above "
                  + ", ".join(f"{t:g}: {s:.4f}" for t, s in zip(agreement.thresholds, agreement.share[a, b])))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
