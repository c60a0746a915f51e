"""The partition that minimises the expected VI or Binder loss, searched on the device (include/sbe_partsearch.h).

consensus.point_estimate and partdist.medoid can only return one of the logged samples; with many objects and noisy
membership no logged sample is close to the centre of the posterior.  This module searches over partitions instead: greedy
single-object reallocation sweeps that minimise the Monte-Carlo expected loss, from many starts, the best result kept (the
sweetening phase of Dahl, Johnson & Mueller 2022; the greedy search of Wade & Ghahramani 2018).  The reference has no tool
for this.

    res = search([run0, run1], loss="vi", starts=16)      # runs: 0/1 [S_r, K, N], disjoint areas
    res.clusters, res.expected_loss, res.medoid_loss       # the estimate uint8 [K, N]; never worse than the medoid
    ev = evaluate([run0, run1], res.clusters)              # ev.vi, ev.binder [n, T]: every sample's distance to an estimate
    ball = credible_ball([run0, run1], res.clusters)       # partdist.CredibleBall around the estimate
    python -m sbayes_amd.partsearch clusters_K3_*.txt --burnin 0.1 --loss vi --out DIR

Contract (tests/_partsearch_oracle.py restates it in NumPy, in the kernel's order; DESIGN.md section 27 states it).  The
samples of all runs after burn-in are concatenated; a sample is a partition into K + 1 blocks, block 0 the objects in no
area.  A candidate is a label row uint8 [N] in 0..K, blocks may be empty.  vi and binder of a candidate against a sample are
partdist's, bit for bit, with the candidate as the earlier partition.  An object step removes object i, scores every block
    VI:     g(q) = T dL[a_q] - 2 S_q,  dL[m] = L[m+1] - L[m],  S_q the sum over t of dL[E_t[q][y[t][i]]] in one fixed tree of
            256 threads (thread j adds t = j, j + 256, .., then the lanes by xor, then the four waves in order);
    Binder: g(0) = 0,  g(q) = T (2 a_q + 1) - 2 sum_{t: y >= 1} (2 E_t[q][y] + 1), exact integers;
chooses the smallest g (the current block among equal values, else the smallest label) and puts i there.  A start sweeps
the objects in its order until a sweep moves nothing, or max_sweeps.  Starts are independent: no output bit depends on how
they are split over calls or how the samples were appended.
Limits: 1 <= K <= 8; N <= 16384; T <= 2^16 samples; max_sweeps <= 1024; the tables of the starts of one library call take
at most 1 GiB (scratch_bytes): the handle splits a longer list over calls.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _clusters, _handle, align, partdist
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_PARTSEARCH_ABI_VERSION of include/sbe_partsearch.h
MAX_CLUSTERS = 8                         # SBE_PARTSEARCH_MAX_CLUSTERS
MAX_OBJECTS = 16384                      # SBE_PARTSEARCH_MAX_OBJECTS
MAX_ROWS = 1 << 16                       # SBE_PARTSEARCH_MAX_ROWS
MAX_SWEEPS = 1024                        # SBE_PARTSEARCH_MAX_SWEEPS
THREADS = 256                            # SBE_PARTSEARCH_THREADS
MAX_SCRATCH_BYTES = 1 << 30              # SBE_PARTSEARCH_MAX_SCRATCH_BYTES
MAX_STARTS = 1 << 16                     # of one search() (the library's own bound is the scratch limit of a call)
LOSSES = partdist.LOSSES                 # index: SBE_PARTSEARCH_LOSS_VI = 0, SBE_PARTSEARCH_LOSS_BINDER = 1

# name -> (restype, argtypes); mirrors include/sbe_partsearch.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_partsearch"),
    "sbe_partsearch_scratch_bytes": (ct.c_int64, [ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_partsearch_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_partsearch_reset": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_partsearch_append_rows": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64]),
    "sbe_partsearch_rows": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int64)]),
    "sbe_partsearch_search": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                         ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_partsearch_evaluate": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_partsearch.h attached."""
    return _handle.bind("sbe_partsearch", PROTOTYPES, ABI_VERSION)


def scratch_bytes(n_clusters, n_samples, n_starts) -> int:
    """Device bytes of the tables of n_starts starts (or candidates): (K + 1)^2 uint16 counts per sample, the samples
    rounded up to 256."""
    padded = (int(n_samples) + THREADS - 1) // THREADS * THREADS
    return int(n_starts) * (int(n_clusters) + 1) ** 2 * padded * 2


def labels_of(clusters):
    """uint8 [.., N]: the block of every object of 0/1 samples [.., K, N] with disjoint areas, 0 for no area, k + 1 for area k."""
    c = np.asarray(clusters)
    k = c.shape[-2]
    return (c.astype(np.uint8) * np.arange(1, k + 1, dtype=np.uint8)[:, None]).sum(axis=-2, dtype=np.uint8)


def rows_of(labels, n_clusters):
    """uint8 [.., K, N] 0/1 rows of label rows [.., N] in 0..K."""
    lab = np.asarray(labels)
    return (lab[..., None, :] == np.arange(1, int(n_clusters) + 1, dtype=lab.dtype)[:, None]).astype(np.uint8)


# ---- validation (host side, before any library call) -----------------------------------------------------------
LIMITS = _clusters.StoreLimits("the partition search", MAX_CLUSTERS, MAX_OBJECTS, MAX_ROWS, rows_why="(2^16 samples)")


def _check_sweeps(max_sweeps):
    max_sweeps = int(max_sweeps)
    if not 1 <= max_sweeps <= MAX_SWEEPS:
        raise ValueError(f"max_sweeps={max_sweeps} out of range [1, {MAX_SWEEPS}]")
    return max_sweeps


def _check_starts(starts):
    starts = int(starts)
    if not 1 <= starts <= MAX_STARTS:
        raise ValueError(f"starts={starts} out of range [1, {MAX_STARTS}]")
    return starts


def _check_labels(name, labels, n_clusters, n_objects):
    """uint8 [n, N] in 0..K of label rows [n, N] or one row [N]."""
    a = np.asarray(labels)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name} must be integer labels, got {a.dtype}")
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != n_objects:
        raise ValueError(f"{name} must be [n, {n_objects}] label rows (at least one), got shape {a.shape}")
    bad = (a < 0) | (a > n_clusters)
    if bad.any():
        s, i = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"{name}[{s}][{i}]={int(a[s, i])} is not a label in [0, {n_clusters}]")
    return np.ascontiguousarray(a, dtype=np.uint8)


def _check_orders(order, n_starts, n_objects):
    """int32 [n_starts, N], every row a permutation of 0..N-1."""
    a = np.asarray(order)
    if a.dtype.kind not in "iu":
        raise TypeError(f"order must be integer, got {a.dtype}")
    if a.ndim == 1:
        a = a[None]
    if a.shape != (n_starts, n_objects):
        raise ValueError(f"order must be [{n_starts}, {n_objects}] (one permutation per start), got shape {a.shape}")
    want = np.arange(n_objects)
    for s in range(n_starts):
        if not np.array_equal(np.sort(a[s]), want):
            raise ValueError(f"order[{s}] is not a permutation of 0 .. {n_objects - 1}")
    return np.ascontiguousarray(a, dtype=np.int32)


@dataclass
class Starts:
    """What the searches of a list of starts ended with, one entry per start: labels uint8 [n, N], sweeps int32, moves int64,
    converged uint8, binder_sum int64, vi_sum float64 (the sums over all samples, both whatever the loss) and trace float64
    [n, max_sweeps] (the loss sum after each sweep, NaN behind the last; None where not asked for)."""
    labels: np.ndarray
    sweeps: np.ndarray
    moves: np.ndarray
    converged: np.ndarray
    binder_sum: np.ndarray
    vi_sum: np.ndarray
    trace: np.ndarray
    kernel_ms: float = 0.0

    def loss_sum(self, loss):
        return self.vi_sum if loss == "vi" else self.binder_sum


@dataclass
class Evaluation:
    """Candidates against every sample: vi float64 and binder int32, each [n, T] (None where not asked for); vi_sum float64
    and binder_sum int64 [n]."""
    vi: np.ndarray
    binder: np.ndarray
    vi_sum: np.ndarray
    binder_sum: np.ndarray
    kernel_ms: float = 0.0

    def distances(self, loss):
        return (self.vi if loss == "vi" else self.binder.astype(np.float64))


class SearchHandle(_handle.UnitHandle):
    """Owner of one sbe_partsearch handle: the label store of the concatenated cluster samples on one device.
    last_kernel_ms(): the kernel of the last library call of search() or evaluate()."""
    _prefix, _noun = "sbe_partsearch", "a partition search handle"

    def __init__(self, device=None):
        self._unshape()
        self._create_on(load, device)

    def _unshape(self):
        self.n_clusters = self.n_objects = self.capacity = 0
        self._stored = 0

    def reset(self, n_clusters, n_objects, capacity):
        """Shape the store: up to `capacity` samples of n_clusters x n_objects bits, empty."""
        n_clusters, n_objects, capacity = int(n_clusters), int(n_objects), int(capacity)
        LIMITS.check_shape(n_clusters, n_objects, capacity)
        self._unshape()
        table = partdist.xlogx(n_objects)
        self._check(self._lib.sbe_partsearch_reset(self._h, n_clusters, n_objects, capacity, _ptr(table)))
        self.n_clusters, self.n_objects, self.capacity = n_clusters, n_objects, capacity

    def _shaped(self, rows=True):
        if not self.n_clusters:
            raise ValueError("the store has no shape yet (reset)")
        if rows and not self._stored:
            raise ValueError("the store holds no samples")

    def append(self, clusters):
        """Append samples ([n, K, N] of 0 / 1 with disjoint areas, or one sample [K, N])."""
        self._shaped(rows=False)
        block = _clusters.check_samples(clusters, (self.n_clusters, self.n_objects))
        if self._stored + block.shape[0] > self.capacity:
            raise ValueError(f"store overflow: the store holds {self._stored} samples, {block.shape[0]} more exceed the capacity of {self.capacity}")
        _clusters.check_disjoint(block)
        _clusters.finish_append(self, self._lib.sbe_partsearch_append_rows(self._h, _ptr(block), block.shape[0]))
        self._stored += block.shape[0]

    def rows(self) -> int:
        n = ct.c_int64(0)
        self._check(self._lib.sbe_partsearch_rows(self._h, ct.byref(n)))
        return n.value

    def per_call(self) -> int:
        """Starts (or candidates) of one library call: their tables stay within MAX_SCRATCH_BYTES."""
        return max(1, MAX_SCRATCH_BYTES // scratch_bytes(self.n_clusters, self._stored, 1))

    def search(self, loss, init, order, max_sweeps=64, trace=False) -> Starts:
        """One search per row of init (label rows [n, N]) with the sweep orders order [n, N], against the stored samples."""
        self._shaped()
        code = LOSSES.index(_clusters.check_loss(loss))
        max_sweeps = _check_sweeps(max_sweeps)
        init = _check_labels("init", init, self.n_clusters, self.n_objects)
        n = init.shape[0]
        order = _check_orders(order, n, self.n_objects)
        out = Starts(np.empty_like(init), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.uint8),
                     np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64), np.empty((n, max_sweeps), dtype=np.float64) if trace else None)
        step = self.per_call()
        for s0 in range(0, n, step):
            part = slice(s0, min(n, s0 + step))
            a_init, a_order, labels, sweeps, moves = init[part], order[part], out.labels[part], out.sweeps[part], out.moves[part]
            converged, binder_sum, vi_sum = out.converged[part], out.binder_sum[part], out.vi_sum[part]
            a_trace = out.trace[part] if trace else None
            self._check(self._lib.sbe_partsearch_search(self._h, code, a_init.shape[0], _ptr(a_init), _ptr(a_order), max_sweeps, _ptr(labels), _ptr(sweeps),
                                                        _ptr(moves), _ptr(converged), _ptr(binder_sum), _ptr(vi_sum), _ptr(a_trace) if trace else None))
            out.kernel_ms += self.last_kernel_ms()
        return out

    def evaluate(self, labels, vi=True, binder=True) -> Evaluation:
        """The label rows [n, N] (or one row [N]) against every stored sample."""
        self._shaped()
        labels = _check_labels("labels", labels, self.n_clusters, self.n_objects)
        n, t = labels.shape[0], self._stored
        out = Evaluation(np.empty((n, t), dtype=np.float64) if vi else None, np.empty((n, t), dtype=np.int32) if binder else None,
                         np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int64))
        step = self.per_call()
        for s0 in range(0, n, step):
            part = slice(s0, min(n, s0 + step))
            a_labels, vi_sum, binder_sum = labels[part], out.vi_sum[part], out.binder_sum[part]
            a_vi, a_binder = out.vi[part] if vi else None, out.binder[part] if binder else None
            self._check(self._lib.sbe_partsearch_evaluate(self._h, a_labels.shape[0], _ptr(a_labels), _ptr(a_vi) if vi else None,
                                                          _ptr(a_binder) if binder else None, _ptr(vi_sum), _ptr(binder_sum)))
            out.kernel_ms += self.last_kernel_ms()
        return out

    @classmethod
    def filled(cls, device, n_clusters, n_objects, blocks):
        """A new handle on `device` that holds the samples of `blocks` one after the other.  The caller closes it."""
        h = cls(device)
        try:
            h.reset(n_clusters, n_objects, max(sum(b.shape[0] for b in blocks), 1))
            for block in blocks:
                if block.shape[0]:
                    h.append(block)
        except BaseException:
            h.close()
            raise
        return h


# ---- the functions ---------------------------------------------------------------------------------------------------
@dataclass
class SearchResult:
    """clusters: the estimate uint8 [K, N] (labels: the same as a label row, 0 for no area); expected_loss: its mean distance to
    the T samples; medoid_loss: that of partdist.medoid's sample; start: the start it came from, -1 for the medoid itself (no
    start was strictly better); converged: whether that start ended with a sweep that moved nothing; starts: per start its
    kind ("medoid", "sample", "zero", "random"), sweeps, moves, converged and loss_sum."""
    clusters: np.ndarray
    labels: np.ndarray
    expected_loss: float
    medoid_loss: float
    loss: str
    n_samples: int
    start: int
    converged: bool
    starts: dict
    kernel_ms: float = 0.0


def make_starts(label_rows, medoid_at, n_clusters, starts, seed):
    """(init uint8 [starts, N], order int32 [starts, N], kinds) of search(): start 0 the medoid under the identity order; of the
    others the first half (rounded up) logged samples drawn by np.random.default_rng(seed), then the all-zero labelling,
    then uniform random labellings; each of them under a seeded permutation."""
    t, n = label_rows.shape
    rng = np.random.default_rng(seed)
    rest = starts - 1
    n_logged = (rest + 1) // 2
    picks = rng.integers(0, t, size=n_logged)
    init = np.zeros((starts, n), dtype=np.uint8)
    order = np.empty((starts, n), dtype=np.int32)
    init[0], order[0] = label_rows[medoid_at], np.arange(n)
    kinds = ["medoid"]
    for s in range(1, starts):
        if s <= n_logged:
            init[s] = label_rows[picks[s - 1]]
            kinds.append("sample")
        elif s == n_logged + 1:
            kinds.append("zero")
        else:
            init[s] = rng.integers(0, n_clusters + 1, size=n)
            kinds.append("random")
        order[s] = rng.permutation(n)
    return init, order, kinds


def rename_blocks(labels, label_rows, n_clusters, loss):
    """The candidate with its blocks renamed by greatest total overlap with the samples' blocks, largest first, ties to the
    smaller label.  Under VI every block takes part; Binder's loss sets block 0 apart, so it stays.  The loss is unaffected."""
    b = n_clusters + 1
    labels = np.asarray(labels)
    per_object = np.stack([(label_rows == l).sum(axis=0) for l in range(b)], axis=1)          # [N, B]: samples with object i in block l
    overlap = np.stack([per_object[labels == q].sum(axis=0) for q in range(b)])               # [B (candidate), B (samples)]
    first = 0 if loss == "vi" else 1
    sizes = np.bincount(labels, minlength=b)
    new = np.arange(b)
    free_q = [q for q in range(first, b) if sizes[q]]
    free_l = list(range(first, b))
    empty_q = [q for q in range(first, b) if not sizes[q]]
    while free_q:
        best = max(((overlap[q, l], -l, -q) for q in free_q for l in free_l))
        q, l = -best[2], -best[1]
        new[q] = l
        free_q.remove(q)
        free_l.remove(l)
    for q, l in zip(empty_q, free_l):                                                           # (empty blocks take what is left)
        new[q] = l
    return new[labels].astype(np.uint8)


def search(runs, loss="vi", starts=16, seed=0, max_sweeps=64, burnin=0.0, device=None) -> SearchResult:
    """The partition with the smallest expected `loss` that greedy single-object sweeps reach from `starts` starts: the best
    of them, or the medoid itself if none is strictly better."""
    loss = _clusters.check_loss(loss)
    starts, max_sweeps, seed = _check_starts(starts), _check_sweeps(max_sweeps), int(seed)
    blocks, k, n = partdist.check_runs(runs, burnin)
    lengths = [b.shape[0] for b in blocks]
    total = sum(lengths)
    partdist.check_sum_rows(total)
    med = partdist.medoid(blocks, loss=loss, device=device)
    label_rows = np.concatenate([labels_of(b) for b in blocks])
    medoid_at = sum(lengths[:med.run]) + med.sample
    init, order, kinds = make_starts(label_rows, medoid_at, k, starts, seed)
    h = SearchHandle.filled(device, k, n, blocks)
    try:
        got = h.search(loss, init, order, max_sweeps)
        sums = got.loss_sum(loss)
        best = min(range(starts), key=lambda s: (sums[s], s))
        labels = got.labels[best]
        if kinds[best] in ("zero", "random"):
            labels = rename_blocks(labels, label_rows, k, loss)
        both = np.stack([label_rows[medoid_at], labels])
        ev = h.evaluate(both, vi=False, binder=False)
        kernel_ms = med.kernel_ms + got.kernel_ms + ev.kernel_ms
    finally:
        h.close()
    final = ev.vi_sum if loss == "vi" else ev.binder_sum
    if not final[1] < final[0]:
        best, labels = -1, label_rows[medoid_at]
    table = dict(kind=kinds, sweeps=got.sweeps, moves=got.moves, converged=got.converged.astype(bool), loss_sum=sums)
    return SearchResult(rows_of(labels, k), labels.copy(), float(final[1 if best >= 0 else 0]) / total, float(final[0]) / total, loss, total, best,
                        bool(got.converged[best]) if best >= 0 else True, table, kernel_ms)


def _check_estimates(estimates, k, n):
    rows = _clusters.check_samples(estimates, (k, n))
    _clusters.check_disjoint(rows)
    return labels_of(rows)


def evaluate(runs, estimates, burnin=0.0, device=None) -> Evaluation:
    """Every sample's distance to each of `estimates` (0/1 [n, K, N] or one [K, N]).  runs: the runs, or a filled SearchHandle."""
    if isinstance(runs, SearchHandle):
        runs._shaped()
        return runs.evaluate(_check_estimates(estimates, runs.n_clusters, runs.n_objects))
    blocks, k, n = partdist.check_runs(runs, burnin)
    partdist.check_sum_rows(sum(b.shape[0] for b in blocks))
    labels = _check_estimates(estimates, k, n)
    h = SearchHandle.filled(device, k, n, blocks)
    try:
        return h.evaluate(labels)
    finally:
        h.close()


def credible_ball(runs, estimate, mass=0.95, loss="vi", burnin=0.0, device=None) -> partdist.CredibleBall:
    """The credible ball around `estimate` (0/1 [K, N], a search's clusters): evaluate's distances per run, the smallest
    distance that holds `mass` of the samples, and which samples lie within."""
    loss, mass = _clusters.check_loss(loss), partdist.check_mass(mass)
    blocks, k, n = partdist.check_runs(runs, burnin)
    partdist.check_sum_rows(sum(b.shape[0] for b in blocks))
    center = _clusters.check_samples(estimate, (k, n))
    if center.shape[0] != 1:
        raise ValueError(f"the estimate must be one sample [{k}, {n}], got {center.shape[0]}")
    ev = evaluate(blocks, center, device=device)
    dist = partdist.split_runs(ev.distances(loss)[0], [b.shape[0] for b in blocks])
    radius = partdist.ball_radius(dist, mass)
    return partdist.CredibleBall(dist, radius, [d <= radius for d in dist], center[0], loss, mass, kernel_ms=ev.kernel_ms)


def main(argv=None):
    ap = _clusters.runs_parser("python -m sbayes_amd.partsearch", "The partition of least expected loss over the cluster samples of several sBayes "
                               "runs: greedy sweeps from many starts, the medoid for comparison and the credible ball around the estimate")
    ap.add_argument("--loss", choices=LOSSES, default="vi")
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-sweeps", type=int, default=64)
    ap.add_argument("--mass", type=float, default=0.95)
    args = ap.parse_args(argv)
    runs, tag, _names, out = _clusters.read_runs(args)
    res = search(runs, loss=args.loss, starts=args.starts, seed=args.seed, max_sweeps=args.max_sweeps, burnin=args.burnin, device=args.device)
    ball = credible_ball(runs, res.clusters, mass=args.mass, loss=args.loss, burnin=args.burnin, device=args.device)
    align.write_clusters(out / f"estimate_{tag}.txt", res.clusters[None])
    inside = sum(int(m.sum()) for m in ball.members)
    print(f"{len(runs)} runs, {res.clusters.shape[0]} clusters, {res.clusters.shape[1]} objects; {res.n_samples} samples after burn-in")
    print(f"expected {args.loss} loss: medoid {res.medoid_loss!r}, search {res.expected_loss!r} "
          f"({'start %d' % res.start if res.start >= 0 else 'no start was better: the medoid'}, {args.starts} starts, "
          f"{'converged' if res.converged else 'not converged'})")
    print(f"credible ball ({args.loss}, mass {ball.mass:g}): radius {ball.radius!r} holds {inside} of {res.n_samples} samples")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
