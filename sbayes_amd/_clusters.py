"""What the units that keep runs of 0/1 cluster samples [S_r, K, N] on the device share on the host side (align, consensus,
partdist, simerr, and partsearch, whose store has no runs): the checks of the samples, the limits of a store and their
messages, the opening of the one-call functions, the handle that owns the store and the command lines' common arguments.
The C side's counterpart is the bit store of csrc/sbe_unit.hip.h (unit_store_limits, unit_bit_store, unit_lanes);
DESIGN.md section 7 describes both."""
from __future__ import annotations

import re
import sys
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle
from ._handle import _ptr

LOSSES = ("vi", "binder")


# ---- validation (host side, before any library call) -----------------------------------------------------------
def check_samples(clusters, shape=None):
    """uint8 [n, K, N] of 0 / 1, C order.  `shape`: the store's (K, N), where one sample [K, N] is accepted too."""
    a = np.asarray(clusters)
    if a.dtype.kind not in "biu":
        raise TypeError(f"cluster samples must be boolean or integer 0 / 1, got {a.dtype}")
    if a.ndim == 2 and shape is not None:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"cluster samples must be [n_samples, n_clusters, n_objects], got shape {a.shape}")
    if shape is not None and a.shape[1:] != tuple(shape):
        raise ValueError(f"samples are {a.shape[1]} clusters x {a.shape[2]} objects, the store holds {shape[0]} x {shape[1]}")
    if a.dtype.kind != "b" and a.size and (a.min() < 0 or a.max() > 1):
        raise ValueError("cluster samples must hold 0 and 1 only")
    return np.ascontiguousarray(a, dtype=np.uint8)


def check_disjoint(block):
    """The areas of every sample of a checked block [n, K, N] are disjoint: the measures are partition measures."""
    if block.size:
        held = block.sum(axis=1, dtype=np.uint8)
        if held.max() > 1:
            s, i = (int(v) for v in np.argwhere(held > 1)[0])
            raise ValueError(f"sample {s}: object {i} is in {int(held[s, i])} areas (the areas of a sample must be disjoint)")


def check_loss(loss):
    if loss not in LOSSES:
        raise ValueError(f"loss={loss!r} is neither 'vi' nor 'binder'")
    return loss


def check_index(word, index):
    """0 or 1: the `word` ("slot", "side") of one of a unit's two results."""
    if isinstance(index, bool) or index not in (0, 1):
        raise ValueError(f"{word}={index!r} is neither 0 nor 1")
    return int(index)


@dataclass(frozen=True)
class StoreLimits:
    """The most a unit's store may be shaped to and the messages that say so: the twin of csrc/sbe_unit.hip.h's
    unit_store_limits.  noun: the store in the messages; max_objects: a number, or a function of K; objects_why, rows_why:
    the reasons in parentheses; max_runs 0: a store without runs (then a shape is K, N, capacity); image_bytes(*shape): the
    device bytes of a shape, at most max_image_bytes."""
    noun: str
    max_clusters: int
    max_objects: object
    max_rows: int
    objects_why: str = ""
    rows_why: str = "(2^20 samples per run)"
    max_runs: int = 0
    image_bytes: object = None
    max_image_bytes: int = 0

    def check_run_count(self, n_runs, fewer=0):
        """`fewer`: runs of the store that the caller needs for itself."""
        if not 1 <= n_runs <= self.max_runs - fewer:
            raise ValueError(f"{n_runs} runs; {self.noun} takes 1 .. {self.max_runs - fewer}")

    def check_ranges(self, *shape):
        if self.max_runs:
            self.check_run_count(shape[0])
        n_clusters, n_objects, capacity = shape[-3:]
        if not 1 <= n_clusters <= self.max_clusters:
            raise ValueError(f"{n_clusters} clusters; {self.noun} takes 1 .. {self.max_clusters}")
        per_k = callable(self.max_objects)
        most = self.max_objects(n_clusters) if per_k else self.max_objects
        if not 1 <= n_objects <= most:
            raise ValueError(f"{n_objects} objects; {f'with {n_clusters} clusters ' if per_k else ''}{self.noun} takes 1 .. {most}"
                             + (" " + self.objects_why if self.objects_why else ""))
        if not 1 <= capacity <= self.max_rows:
            raise ValueError(f"capacity={capacity} out of range [1, {self.max_rows}] {self.rows_why}")

    def check_image(self, n_runs, n_clusters, n_objects, capacity, *more, how=""):
        """more: what image_bytes takes behind the shape; how: what the message says of it."""
        need = self.image_bytes(n_runs, n_clusters, n_objects, capacity, *more)
        if need > self.max_image_bytes:
            raise ValueError(f"a store of {n_runs} runs x {capacity} samples x {n_clusters} clusters x {n_objects} objects{how} takes {need} "
                             f"bytes on the device, the limit is {self.max_image_bytes}")

    def check_shape(self, *shape):
        self.check_ranges(*shape)
        if self.image_bytes is not None:
            self.check_image(*shape)


# ---- the opening of the one-call functions -------------------------------------------------------------------------
def store_shape(blocks, k, n):
    """The shape of a store that holds these runs: the capacity is the longest run's, and at least one sample."""
    return len(blocks), k, n, max(max(b.shape[0] for b in blocks), 1)


def check_runs(limits, runs, fewer_runs=0):
    """(the runs uint8 [S_r, K, N] in C order, K, N) of a list of runs: their number within the limits, every run's samples,
    one K and one N.  The caller goes on with limits.check_shape(*store_shape(..)) and after_burnin() in its unit's order."""
    runs = list(runs)
    limits.check_run_count(len(runs), fewer_runs)
    blocks = [check_samples(r) for r in runs]
    if len({b.shape[1:] for b in blocks}) != 1:
        raise ValueError(f"the runs differ in clusters or objects: {[b.shape[1:] for b in blocks]}")
    return (blocks, *blocks[0].shape[1:])


def burn_rows(lengths, burnin):
    burnin = float(burnin)
    if not 0.0 <= burnin < 1.0:
        raise ValueError(f"burnin={burnin} must lie in [0, 1)")
    return [int(burnin * int(s)) for s in lengths]                          # Results.drop_burnin


def after_burnin(blocks, burnin):
    return [b[at:] for b, at in zip(blocks, burn_rows([b.shape[0] for b in blocks], burnin))]


def argmin_rows(values):
    """(run, sample) of the smallest (value, run, sample) over per-run arrays of scores or losses."""
    best = None
    for r, s in enumerate(values):
        if len(s):
            at = int(np.argmin(s))                                          # (the first minimum)
            if best is None or s[at] < best[0]:
                best = (s[at], r, at)
    if best is None:
        raise ValueError("no sample to choose from")
    return best[1], best[2]


# ---- the handle --------------------------------------------------------------------------------------------------
def finish_append(h, rc):
    """The code of an append_rows on a store with an operand image.  SBE_ERR_HIP: a piece may be half in the image, the
    library has unshaped the store, and so does this object."""
    if rc == 2:
        message = h._last_error()
        h._unshape()
        raise _handle.EngineError(rc, message)
    h._check(rc)


class SampleStoreHandle(_handle.RowStoreHandle):
    """Owner of a handle with the store of several runs of cluster samples on one device.  The unit's module has load(); the
    class names its entry points (_prefix, _noun) and its limits (_limits), and where the unit keeps results of the store
    (consensus' slots, simerr's sides) it forgets in _out_of_date() what they hold."""
    _lane = "run"
    _limits = None

    def __init__(self, device=None):
        self._unshape()
        self._create_on(sys.modules[type(self).__module__].load, device)

    def _lane_count(self):
        return self.n_runs

    def _unshape(self):
        self.n_runs = self.n_clusters = self.n_objects = self.capacity = 0
        self._stored = []
        self._out_of_date()

    def _out_of_date(self):
        pass

    def _check_shape(self, *shape):
        self._limits.check_shape(*shape)

    def _behind_shape(self, shape, extra):
        """What <prefix>_reset takes behind the checked shape (numbers, or arrays whose addresses go): the trailing arguments
        of reset() as they are."""
        return extra

    def reset(self, n_runs, n_clusters, n_objects, capacity, *extra):
        """Shape the store: n_runs empty runs of up to `capacity` samples of n_clusters x n_objects bits.  extra: the whole
        numbers a unit's shape has more (simerr: batch_rows)."""
        shape = tuple(int(v) for v in (n_runs, n_clusters, n_objects, capacity))
        extra = tuple(int(v) for v in extra)
        self._check_shape(*shape, *extra)
        self._unshape()
        behind = self._behind_shape(shape, extra)
        self._check(self._fn("reset")(self._h, *shape, *(_ptr(v) if isinstance(v, np.ndarray) else v for v in behind)))
        self.n_runs, self.n_clusters, self.n_objects, self.capacity = shape
        self._stored = [0] * shape[0]

    def _shaped(self):
        if not self.n_runs:
            raise ValueError("the store has no shape yet (reset)")

    def _checked_block(self, run, clusters):
        """(run, samples uint8 [n, K, N]) of an append, refused here where the run would overflow."""
        run = self._check_lane(run)
        block = check_samples(clusters, (self.n_clusters, self.n_objects))
        if self._stored[run] + block.shape[0] > self.capacity:
            raise ValueError(f"store overflow: run {run} holds {self._stored[run]} samples, {block.shape[0]} more exceed the capacity "
                             f"of {self.capacity}")
        return run, block

    def _check_block(self, block):
        """The unit's own check of the samples of an append (partdist: disjoint areas)."""

    def append(self, run, clusters):
        """Append samples ([n, K, N] of 0 / 1, or one sample [K, N]) to a run.  What the unit has computed from the store is
        out of date afterwards."""
        run, block = self._checked_block(run, clusters)
        self._check_block(block)
        if block.shape[0]:
            self._out_of_date()
        finish_append(self, self._append_rows(run, block))
        self._stored[run] += block.shape[0]

    def set_launch_tiles(self, tile_pairs):
        """Tiles (tile pairs) per launch of the unit's kernel on the matrix pipe (0: the default); the results do not depend
        on it."""
        self._check(self._fn("set_launch_tiles")(self._h, int(tile_pairs)))

    def _mask(self, runs):
        """uint8 [R]: 1 for the selected runs (indices; None: every run)."""
        mask = np.zeros(self.n_runs, dtype=np.uint8)
        for run in (range(self.n_runs) if runs is None else runs):
            mask[self._check_lane(run)] = 1
        return mask


# ---- the command lines ---------------------------------------------------------------------------------------------
def runs_parser(prog, description):
    """The parser of a command line over the clusters files of several runs: the files, --burnin, --out and --device.  The
    program adds its own options."""
    import argparse
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument("files", nargs="+", type=Path, help="clusters files of the runs (clusters_K<k>_<run>.txt), all of one K")
    ap.add_argument("--burnin", type=float, default=0.0)
    ap.add_argument("--out", type=Path, default=None, help="folder of the outputs (default: that of the first file)")
    ap.add_argument("--device", type=int, default=None)
    return ap


def read_runs(args):
    """(runs uint8 [S_r, K, N], tag, names, out) of the files runs_parser's arguments name: the tag K<k> of the first file's
    name (else of its samples), the run names of the file names (else the runs' numbers), and the output folder, made here."""
    from . import align
    runs = [align.read_clusters(p) for p in args.files]
    if len({c.shape[1:] for c in runs}) != 1:
        raise SystemExit(f"the files differ in clusters or objects: {[c.shape[1:] for c in runs]}")
    m = re.match(r"clusters_(K\d+)_", args.files[0].name)
    tag = m.group(1) if m else f"K{runs[0].shape[1]}"
    names = []
    for r, p in enumerate(args.files):
        m = re.match(r"clusters_K\d+_(.*)\.txt$", p.name)
        names.append(m.group(1) if m else str(r))
    out = args.files[0].parent if args.out is None else args.out
    out.mkdir(parents=True, exist_ok=True)
    return runs, tag, names, out
