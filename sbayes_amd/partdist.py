"""Pairwise distances between cluster samples, on the device (include/sbe_partdist.h).

consensus reduces a posterior to one [N, N] matrix before anything is compared.  This module compares the samples with
each other, with no label matching and without averaging them away first: Binder's distance, the variation of information
(Meila) and the adjusted Rand index of every pair of samples, and what is read from them -- whether the runs explore the
same region of partition space (within-run against between-run distance), the point estimate under a loss other than
Binder's (the medoid; Wade & Ghahramani 2018), the credible ball around it and a label-free trace per sample that
diag.convergence can take.  The reference has no tool for this.

    d = distances([run0, run1], burnin=0.1)               # runs: 0/1 [S_r, K, N], disjoint areas; d.binder, d.vi, d.ari [T, T]
    est = medoid([run0, run1], loss="vi")                 # est.run, est.sample, est.clusters [K, N], est.expected_loss
    rd = run_distances([run0, run1, run2])                # rd.vi, rd.binder: float64 [R, R] mean distances
    ball = credible_ball([run0, run1], mass=0.95)         # ball.distances (per run), ball.radius, ball.members
    python -m sbayes_amd.partdist clusters_K3_*.txt --burnin 0.1 --loss vi --mass 0.95 --out DIR

Contract (tests/_partdist_oracle.py restates it in NumPy; DESIGN.md section 23 states it).  A sample is a partition of the
N objects into K + 1 blocks, block 0 the objects in no area; samples are ordered by (run, sample).  For samples x and y
with the table n[k][l] = |x_k & y_l| and the area sizes a, b, the extended table E [K+1][K+1] adds block 0 of each side:
    binder(x,y) = sum a^2 + sum b^2 - 2 sum n^2, int32, exact: the ordered object pairs that share an area in exactly one
                  of the two; for a selection with similarity counts C, sum_t binder(s,t) = score[s] + sum C (consensus);
    sumsq(x,y)  = sum E^2, int32: with the sizes, what the Rand and adjusted Rand index need (adjusted_rand);
    vi(x,y)     = max(0, ((h_x + h_y) - 2 j) / N) in nats, x the earlier sample, h = sum_k L[a+_k], j = sum_kl L[E[k][l]] (k
                  major), every sum left to right from 0.0 in float64, L[m] = m log m the table xlogx(N) handed to the device:
                  device and checker agree bit for bit.  Exactly 0.0 for the same blocks under the same labels.
    sums        binder_sum[s][r'] int64 exact, vi_sum[s][r'] float64 in one tree: 64 lanes, lane j adds t = j, j + 64, .. onto
                  0.0, then xor exchanges at distances 32 .. 1.
Limits: 1 <= K <= 8; N <= 16384; at most 64 runs of at most 2^20 samples; a store of at most 16 GiB on the device
(image_bytes); a block of at most 2^28 entries; at most 2^16 samples in a selection for the sums.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import math
from dataclasses import dataclass

import numpy as np

from . import _clusters, _handle, align
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_PARTDIST_ABI_VERSION of include/sbe_partdist.h
MAX_CLUSTERS = 8                         # SBE_PARTDIST_MAX_CLUSTERS
MAX_OBJECTS = 16384                      # SBE_PARTDIST_MAX_OBJECTS
MAX_RUNS = 64                            # SBE_PARTDIST_MAX_RUNS
MAX_ROWS = 1 << 20                       # SBE_PARTDIST_MAX_ROWS
ROUND = 256                              # SBE_PARTDIST_ROUND
MAX_IMAGE_BYTES = 1 << 34                # SBE_PARTDIST_MAX_IMAGE_BYTES
MAX_BLOCK = 1 << 28                      # SBE_PARTDIST_MAX_BLOCK
MAX_SUM_ROWS = 1 << 16                   # SBE_PARTDIST_MAX_SUM_ROWS
MAX_PAIRS = 1 << 24                      # SBE_PARTDIST_MAX_PAIRS
LOSSES = _clusters.LOSSES

# name -> (restype, argtypes); mirrors include/sbe_partdist.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.store_prototypes("sbe_partdist", [ct.c_int, ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_partdist_image_bytes": (ct.c_int64, [ct.c_int, ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_partdist_sizes": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p]),
    "sbe_partdist_block": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p,
                                      ct.c_void_p]),
    "sbe_partdist_sums": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_partdist_tables": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_void_p]),
    "sbe_partdist_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
}


def load():
    """The engine library with the prototypes of include/sbe_partdist.h attached."""
    return _handle.bind("sbe_partdist", PROTOTYPES, ABI_VERSION)


def padded_clusters(n_clusters) -> int:
    """K_pad: the power of two >= K (a sample takes K_pad rows of the operand image)."""
    return 1 << (int(n_clusters) - 1).bit_length()


def image_bytes(n_runs, n_clusters, n_objects, capacity) -> int:
    """Device bytes of a store of this shape: the FP4 operand image (per run capacity K_pad rows, rounded up to whole tiles
    of 32, of N rounded up to 256 objects, a nibble each) plus the bit rows."""
    words = (int(n_objects) + 31) // 32
    rows = (int(capacity) * padded_clusters(n_clusters) + 31) // 32 * 32
    row_bytes = (int(n_objects) + ROUND - 1) // ROUND * (ROUND // 2)
    return int(n_runs) * rows * row_bytes + int(n_runs) * int(capacity) * int(n_clusters) * words * 4


def xlogx(n_objects):
    """float64 [N + 1]: L[0] = 0, L[m] = m log m -- the table the device adds up (it never takes a log itself)."""
    m = np.arange(int(n_objects) + 1, dtype=np.float64)
    table = np.zeros(int(n_objects) + 1, dtype=np.float64)
    table[1:] = m[1:] * np.log(m[1:])
    return table


# ---- validation (host side, before any library call) -----------------------------------------------------------
LIMITS = _clusters.StoreLimits("the partition store", MAX_CLUSTERS, MAX_OBJECTS, MAX_ROWS, "(2 N^2 fits an int32)", max_runs=MAX_RUNS,
                               image_bytes=image_bytes, max_image_bytes=MAX_IMAGE_BYTES)


def check_runs(runs, burnin, extra_runs=0):
    """The runs after burn-in (uint8 [S_r, K, N], C order, disjoint areas), K, N.  extra_runs: runs of the store that the
    caller keeps for itself."""
    blocks, k, n = _clusters.check_runs(LIMITS, runs, extra_runs)
    LIMITS.check_shape(*_clusters.store_shape(blocks, k, n))
    blocks = _clusters.after_burnin(blocks, burnin)
    if sum(b.shape[0] for b in blocks) < 1:
        raise ValueError("the runs hold no samples")
    for b in blocks:
        _clusters.check_disjoint(b)
    return blocks, k, n


def check_sum_rows(total):
    if total < 1:
        raise ValueError("the selected runs hold no samples")
    if total > MAX_SUM_ROWS:
        raise ValueError(f"the selection holds {total} samples, the limit for the sums is {MAX_SUM_ROWS} (2^16)")


@dataclass
class Block:
    """The measures of a block of sample pairs, dense [n_rows, n_cols]; None where not asked for."""
    binder: np.ndarray
    vi: np.ndarray
    sumsq: np.ndarray


class PartitionHandle(_clusters.SampleStoreHandle):
    """Owner of one sbe_partdist handle: the store of several runs of cluster samples with disjoint areas on one device.
    last_kernel_ms(): the kernels of the last block(), sums() or tables()."""
    _prefix, _noun, _limits = "sbe_partdist", "a partition handle", LIMITS

    def _behind_shape(self, shape, extra):
        return (xlogx(shape[2]),)

    def _check_block(self, block):
        _clusters.check_disjoint(block)

    def _check_range(self, side, run, first, count):
        run = self._check_lane(run)
        first = int(first)
        count = self._stored[run] - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self._stored[run]:
            raise ValueError(f"{side}s [{first}, {first} + {count}) are not within the {self._stored[run]} samples of run {run} (at least one)")
        return run, first, count

    def sizes(self, run):
        """int32 [rows(run), K]: the area sizes of every stored sample of a run."""
        self._shaped()
        run = self._check_lane(run)
        sizes = np.empty((self._stored[run], self.n_clusters), dtype=np.int32)
        self._check(self._lib.sbe_partdist_sizes(self._h, run, _ptr(sizes)))
        return sizes

    def block(self, row_run, row_first=0, n_rows=None, col_run=None, col_first=0, n_cols=None, binder=True, vi=True, sumsq=True) -> Block:
        """The measures of the samples [row_first, row_first + n_rows) of row_run against [col_first, col_first + n_cols) of
        col_run (None: row_run); a count of None runs to the end of the run."""
        self._shaped()
        row_run, row_first, n_rows = self._check_range("row", row_run, row_first, n_rows)
        col_run, col_first, n_cols = self._check_range("col", row_run if col_run is None else col_run, col_first, n_cols)
        if n_rows * n_cols > MAX_BLOCK:
            raise ValueError(f"a block of {n_rows} x {n_cols} = {n_rows * n_cols} entries, the limit is {MAX_BLOCK} (2^28)")
        if not (binder or vi or sumsq):
            raise ValueError("at least one of binder, vi and sumsq is needed")
        out_b = np.empty((n_rows, n_cols), dtype=np.int32) if binder else None
        out_v = np.empty((n_rows, n_cols), dtype=np.float64) if vi else None
        out_s = np.empty((n_rows, n_cols), dtype=np.int32) if sumsq else None
        self._check(self._lib.sbe_partdist_block(self._h, row_run, row_first, n_rows, col_run, col_first, n_cols, _ptr(out_b) if binder else None,
                                                 _ptr(out_v) if vi else None, _ptr(out_s) if sumsq else None))
        return Block(out_b, out_v, out_s)

    def sums(self, runs=None):
        """(binder_sum int64, vi_sum float64), each [T_sel, R_sel]: for every sample of the selected runs (indices; None: every
        run), in (run, sample) order, the sum of its distances to the samples of each selected run."""
        self._shaped()
        mask = self._mask(runs)
        total = sum(s for s, m in zip(self._stored, mask) if m)
        check_sum_rows(total)
        binder_sum = np.empty((total, int(mask.sum())), dtype=np.int64)
        vi_sum = np.empty((total, int(mask.sum())), dtype=np.float64)
        self._check(self._lib.sbe_partdist_sums(self._h, _ptr(mask), _ptr(binder_sum), _ptr(vi_sum)))
        return binder_sum, vi_sum

    def tables(self, pairs):
        """int32 [n_pairs, K, K]: the raw tables n[k][l] of the listed pairs [n_pairs, 4] (run, sample, run, sample), counted
        from the bit rows on the vector pipe."""
        self._shaped()
        pairs = np.ascontiguousarray(pairs, dtype=np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 4 or not 1 <= pairs.shape[0] <= MAX_PAIRS:
            raise ValueError(f"pairs must be [n_pairs, 4] (run, sample, run, sample) with 1 .. {MAX_PAIRS} pairs, got shape {pairs.shape}")
        stored = np.array(self._stored, dtype=np.int64)
        for side in (0, 2):
            run, row = pairs[:, side], pairs[:, side + 1]
            bad = (run < 0) | (run >= self.n_runs)
            bad |= (row < 0) | (row >= stored[np.where(bad, 0, run)])
            if bad.any():
                p = int(np.flatnonzero(bad)[0])
                raise ValueError(f"pairs[{p}]: (run {int(run[p])}, sample {int(row[p])}) is not a stored sample")
        tables = np.empty((pairs.shape[0], self.n_clusters, self.n_clusters), dtype=np.int32)
        self._check(self._lib.sbe_partdist_tables(self._h, _ptr(pairs), pairs.shape[0], _ptr(tables)))
        return tables


# ---- host-side arithmetic ------------------------------------------------------------------------------------------
def _pair_counts(sizes, n_objects):
    """int64 [..]: twice the number of object pairs within the K + 1 blocks, sum a+^2 - N, from area sizes [.., K]."""
    sizes = np.asarray(sizes, dtype=np.int64)
    outside = int(n_objects) - sizes.sum(axis=-1)
    return (sizes * sizes).sum(axis=-1) + outside * outside - int(n_objects)


def rand_index(sumsq, sizes_a, sizes_b, n_objects):
    """The Rand index of the (K+1)-block partitions: float64 [R, C] from sumsq [R, C] and the area sizes [R, K], [C, K];
    1.0 for a single object."""
    n = int(n_objects)
    both = np.asarray(sumsq, dtype=np.int64) - n                               # 2 sum C(E, 2)
    a, b = _pair_counts(sizes_a, n)[..., :, None], _pair_counts(sizes_b, n)[..., None, :]
    pairs = n * (n - 1)                                                        # 2 C(N, 2)
    if pairs == 0:
        return np.ones(np.broadcast(both, a, b).shape)
    return (pairs + 2 * both - a - b) / float(pairs)


def adjusted_rand(sumsq, sizes_a, sizes_b, n_objects):
    """The adjusted Rand index (Hubert & Arabie) of the (K+1)-block partitions: float64 [R, C] from sumsq [R, C] and the
    area sizes [R, K], [C, K].  Numerator and denominator are exact integers, divided once; a denominator of 0 (both
    partitions have one block, or every block is one object) gives 1.0."""
    n = int(n_objects)
    both = np.asarray(sumsq, dtype=np.int64) - n                               # 2 sum C(E, 2)            <= 2^28
    a, b = _pair_counts(sizes_a, n)[..., :, None], _pair_counts(sizes_b, n)[..., None, :]
    pairs = n * (n - 1)                                                        # 2 C(N, 2)                <= 2^28
    # (index - expected) / (mean - expected) with index = both / 2, expected = (a / 2)(b / 2) / (pairs / 2), mean = (a + b) / 4,
    # all times 4 pairs: every product stays below 2^58
    num = 2 * both * pairs - 2 * a * b
    den = (a + b) * pairs - 2 * a * b
    out = np.ones(np.broadcast(num, den).shape)
    np.divide(num, den, out=out, where=den != 0)
    return out


argmin_loss = _clusters.argmin_rows       # (run, sample) of the smallest (loss, run, sample) over per-run loss arrays


def split_runs(rows, lengths):
    at = np.cumsum([0] + list(lengths))
    return [rows[at[r]:at[r + 1]] for r in range(len(lengths))]


def _total_loss(binder_sum, vi_sum, lengths, loss):
    """Per run, every sample's summed distance to all samples: int64 for binder; float64 for vi, the runs added in order."""
    if loss == "binder":
        total = binder_sum.sum(axis=1)
    else:
        total = np.zeros(vi_sum.shape[0])
        for col in range(vi_sum.shape[1]):
            total = total + vi_sum[:, col]
    return split_runs(total, lengths)


def mean_run_distances(binder_sum, vi_sum, lengths):
    """(binder, vi) float64 [R, R] from the sums of all runs: the mean distance of a sample of run r to a sample of run r';
    on the diagonal the zero self-pairs are left out (nan for a run of one sample, or of none).  Python integers for binder."""
    r_n = len(lengths)
    binder, vi = np.full((r_n, r_n), np.nan), np.full((r_n, r_n), np.nan)
    rows_b, rows_v = split_runs(binder_sum, lengths), split_runs(vi_sum, lengths)
    for a in range(r_n):
        for b in range(r_n):
            pairs = lengths[a] * (lengths[a] - 1) if a == b else lengths[a] * lengths[b]
            if pairs:
                binder[a, b] = sum(int(v) for v in rows_b[a][:, b]) / pairs
                vi[a, b] = math.fsum(rows_v[a][:, b]) / pairs
    return binder, vi


def ball_radius(distances, mass):
    """The smallest distance d such that at least `mass` of the samples lie within d."""
    d = np.sort(np.concatenate([np.asarray(v, dtype=np.float64) for v in distances]))
    if not d.size:
        raise ValueError("no sample to choose from")
    return float(d[max(int(math.ceil(mass * d.size)) - 1, 0)])


# ---- the functions ---------------------------------------------------------------------------------------------------
@dataclass
class Distances:
    """binder int32, vi float64 (nats) and ari float64, each [T, T] over the samples of all runs in (run, sample) order;
    sizes: int32 [T, K]; offsets: the first sample of every run, and T."""
    binder: np.ndarray
    vi: np.ndarray
    ari: np.ndarray
    sizes: np.ndarray
    offsets: tuple
    kernel_ms: float = 0.0


@dataclass
class Medoid:
    """The sample with the smallest expected loss: run and sample (counted after burn-in), its clusters uint8 [K, N];
    expected_loss: one float64 array per run, the mean distance of every sample to all T samples."""
    run: int
    sample: int
    clusters: np.ndarray
    expected_loss: list
    loss: str
    n_samples: int
    kernel_ms: float = 0.0


@dataclass
class RunDistances:
    """binder, vi: float64 [R, R] mean distances between the samples of two runs; the diagonal is within-run and leaves the
    zero self-pairs out.  n_samples: per run."""
    binder: np.ndarray
    vi: np.ndarray
    n_samples: tuple
    kernel_ms: float = 0.0


@dataclass
class CredibleBall:
    """distances: one float64 array per run, every sample's distance to the estimate; radius: the smallest distance that
    holds `mass` of the samples; members: one boolean array per run (distance <= radius); estimate: uint8 [K, N]."""
    distances: list
    radius: float
    members: list
    estimate: np.ndarray
    loss: str
    mass: float
    run: int = -1                        # of the estimate, where it is a sample of the runs (the medoid)
    sample: int = -1
    kernel_ms: float = 0.0


def _filled(blocks, k, n, device, extra=None):
    shape = list(_clusters.store_shape(blocks, k, n))
    if extra is not None:
        shape[0] += 1
    h = PartitionHandle.filled(device, shape, blocks)
    try:
        if extra is not None:
            h.append(len(blocks), extra)
    except BaseException:
        h.close()
        raise
    return h


def distances(runs, burnin=0.0, device=None) -> Distances:
    """Binder's distance, the variation of information and the adjusted Rand index of every pair of samples of `runs` (a
    list of 0/1 [S_r, K, N] arrays with disjoint areas) after burn-in."""
    blocks, k, n = check_runs(runs, burnin)
    lengths = [b.shape[0] for b in blocks]
    total = sum(lengths)
    if total * total > MAX_BLOCK:
        raise ValueError(f"{total} samples make {total * total} pairs, the limit is {MAX_BLOCK} (2^28): use block() or sums() of a PartitionHandle")
    at = np.cumsum([0] + lengths)
    binder, vi = np.empty((total, total), dtype=np.int32), np.empty((total, total), dtype=np.float64)
    sumsq = np.empty((total, total), dtype=np.int32)
    kernel_ms = 0.0
    h = _filled(blocks, k, n, device)
    try:
        sizes = np.concatenate([h.sizes(r) for r in range(len(blocks))])
        for a in range(len(blocks)):
            for b in range(len(blocks)):
                if lengths[a] and lengths[b]:
                    got = h.block(a, col_run=b)
                    kernel_ms += h.last_kernel_ms()
                    binder[at[a]:at[a + 1], at[b]:at[b + 1]] = got.binder
                    vi[at[a]:at[a + 1], at[b]:at[b + 1]] = got.vi
                    sumsq[at[a]:at[a + 1], at[b]:at[b + 1]] = got.sumsq
    finally:
        h.close()
    return Distances(binder, vi, adjusted_rand(sumsq, sizes, sizes, n), sizes, tuple(int(v) for v in at), kernel_ms)


def _sums_of(blocks, k, n, device):
    check_sum_rows(sum(b.shape[0] for b in blocks))
    h = _filled(blocks, k, n, device)
    try:
        binder_sum, vi_sum = h.sums()
        return binder_sum, vi_sum, h.last_kernel_ms()
    finally:
        h.close()


def medoid(runs, loss="vi", burnin=0.0, device=None) -> Medoid:
    """The point estimate under `loss`: the sample of `runs` (after burn-in) with the smallest (summed distance to all
    samples, run, sample).  For loss="binder" it is consensus.point_estimate's sample."""
    loss = _clusters.check_loss(loss)
    blocks, k, n = check_runs(runs, burnin)
    lengths = [b.shape[0] for b in blocks]
    binder_sum, vi_sum, kernel_ms = _sums_of(blocks, k, n, device)
    totals = _total_loss(binder_sum, vi_sum, lengths, loss)
    run, sample = argmin_loss(totals)
    return Medoid(run, sample, blocks[run][sample].copy(), [t / float(sum(lengths)) for t in totals], loss, sum(lengths), kernel_ms)


def run_distances(runs, burnin=0.0, device=None) -> RunDistances:
    """Mean distances between the samples of every two runs: within-run on the diagonal, between-run off it."""
    blocks, k, n = check_runs(runs, burnin)
    lengths = [b.shape[0] for b in blocks]
    binder_sum, vi_sum, kernel_ms = _sums_of(blocks, k, n, device)
    binder, vi = mean_run_distances(binder_sum, vi_sum, lengths)
    return RunDistances(binder, vi, tuple(lengths), kernel_ms)


def check_mass(mass):
    mass = float(mass)
    if not 0.0 < mass <= 1.0:
        raise ValueError(f"mass={mass} must lie in (0, 1]")
    return mass


def _distances_to(h, lengths, at, loss, clock=lambda: 0.0):
    """(one float64 array per run of `lengths`: every sample's distance to the stored sample at = (run, sample); the kernels'
    time) on a filled handle.  clock: the handle's last_kernel_ms where the caller wants that time."""
    dist, kernel_ms = [], 0.0
    for r in range(len(lengths)):
        if lengths[r]:
            got = h.block(r, col_run=at[0], col_first=at[1], n_cols=1, binder=loss == "binder", vi=loss == "vi", sumsq=False)
            kernel_ms += clock()
            dist.append((got.vi if loss == "vi" else got.binder)[:, 0].astype(np.float64))
        else:
            dist.append(np.zeros(0))
    return dist, kernel_ms


def credible_ball(runs, estimate=None, mass=0.95, loss="vi", burnin=0.0, device=None) -> CredibleBall:
    """The credible ball around `estimate` (0/1 [K, N]; None: the medoid under `loss`): every sample's distance to it, the
    smallest distance that holds `mass` of the samples, and which samples lie within."""
    loss, mass = _clusters.check_loss(loss), check_mass(mass)
    given = estimate is not None
    blocks, k, n = check_runs(runs, burnin, extra_runs=int(given))
    lengths = [b.shape[0] for b in blocks]
    extra = None
    if given:
        extra = _clusters.check_samples(estimate, (k, n))
        if extra.shape[0] != 1:
            raise ValueError(f"the estimate must be one sample [{k}, {n}], got {extra.shape[0]}")
        _clusters.check_disjoint(extra)
    else:
        check_sum_rows(sum(lengths))
    h = _filled(blocks, k, n, device, extra)
    kernel_ms = 0.0
    try:
        if given:
            run, sample, at = -1, -1, (len(blocks), 0)
        else:
            binder_sum, vi_sum = h.sums(range(len(blocks)))
            kernel_ms += h.last_kernel_ms()
            at = run, sample = argmin_loss(_total_loss(binder_sum, vi_sum, lengths, loss))
        dist, block_ms = _distances_to(h, lengths, at, loss, h.last_kernel_ms)
        kernel_ms += block_ms
    finally:
        h.close()
    radius = ball_radius(dist, mass)
    center = extra[0] if given else blocks[run][sample].copy()
    return CredibleBall(dist, radius, [d <= radius for d in dist], center, loss, mass, run, sample, kernel_ms)


# ---- files -------------------------------------------------------------------------------------------------------
def write_trace(path, distances, loss):
    """One distance per sample under a header line: readable as a column by diag (repr of float64: reads back bit for bit)."""
    with open(path, "w") as f:
        f.write(f"{loss}_to_estimate\n")
        for v in distances:
            f.write(repr(float(v)) + "\n")


def main(argv=None):
    ap = _clusters.runs_parser("python -m sbayes_amd.partdist", "Pairwise distances between the cluster samples of several sBayes runs: the "
                               "medoid under the variation of information or Binder's loss, run-against-run distances and the credible ball")
    ap.add_argument("--loss", choices=LOSSES, default="vi")
    ap.add_argument("--mass", type=float, default=0.95)
    args = ap.parse_args(argv)
    runs, tag, names, out = _clusters.read_runs(args)
    mass = check_mass(args.mass)
    blocks, k, n = check_runs(runs, args.burnin)
    lengths = [b.shape[0] for b in blocks]
    check_sum_rows(sum(lengths))
    h = _filled(blocks, k, n, args.device)                   # one store serves the three questions
    try:
        binder_sum, vi_sum = h.sums()
        run, sample = argmin_loss(_total_loss(binder_sum, vi_sum, lengths, args.loss))
        dist, _ms = _distances_to(h, lengths, (run, sample), args.loss)
    finally:
        h.close()
    mean_binder, mean_vi = mean_run_distances(binder_sum, vi_sum, lengths)
    radius = ball_radius(dist, mass)
    inside = sum(int((d <= radius).sum()) for d in dist)
    print(f"{len(blocks)} runs, {k} clusters, {n} objects; {sum(lengths)} samples after burn-in")
    print(f"medoid ({args.loss}): sample {sample} (after burn-in) of {args.files[run].name}")
    align.write_clusters(out / f"medoid_{tag}.txt", blocks[run][sample][None])
    for r, name in enumerate(names):
        write_trace(out / f"partition_trace_{tag}_{name}.txt", dist[r], args.loss)
    table = mean_vi if args.loss == "vi" else mean_binder
    print(f"mean {args.loss} distance between the samples of two runs (the diagonal: within the run, without the self-pairs):")
    for a in range(len(blocks)):
        print(f"{args.files[a].name}\t" + "\t".join("%.6f" % table[a, b] for b in range(len(blocks))))
    print(f"credible ball ({args.loss}, mass {mass:g}): radius {radius!r} holds {inside} of {sum(lengths)} samples")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
