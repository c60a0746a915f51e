"""CPU checks of what the handles that store cluster samples share (sbayes_amd/_clusters.py, SampleStoreHandle and the tail of
SearchHandle.append): what reset hands the library, what a failed append leaves behind, when a unit's results go out of date,
the mask of a selection, the refusals that are made before any library call, and the command lines' reader.  A fake library,
no device."""
import ctypes as ct
import os
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _clusters, _handle, align, consensus, partdist, partsearch, simerr
from sbayes_amd._handle import _ptr
from tests import _abi_header as abi

R, K, N, CAP = 2, 3, 33, 7
# class, what its reset takes behind (R, K, N, CAP), the attribute that holds what the unit has computed from the store, the word of its index
RUN_STORES = [(align.AlignHandle, (), None, None), (consensus.ConsensusHandle, (), "slot_samples", "slot"),
              (partdist.PartitionHandle, (), None, None), (simerr.SimErrHandle, (2,), "side_batches", "side")]
STORES = RUN_STORES + [(partsearch.SearchHandle, (), None, None)]
IDS = [c[0].__name__ for c in STORES]


def _fake(cls, monkeypatch, append_code=0):
    """A handle of `cls` on a library that records its calls as (name, args) and whose append_rows returns `append_code`, under
    a create that touches no device."""
    calls = []

    def entry(name, code=0):
        def fn(*args):
            calls.append((name, args))
            return code
        return fn
    names = {"reset", "rows", "destroy", "last_kernel_ms", "set_launch_tiles"}
    lib = SimpleNamespace(**{f"{cls._prefix}_{name}": entry(name) for name in names},
                          **{f"{cls._prefix}_append_rows": entry("append_rows", append_code), f"{cls._prefix}_last_error": lambda h: b"refused"})

    def create_on(self, load, device):
        self._h, self._lib, self._pid, self.device = ct.c_void_p(1), lib, os.getpid(), device
    monkeypatch.setattr(cls, "_create_on", create_on)
    return cls(0), calls


def _runs(cls):
    return cls is not partsearch.SearchHandle


def _reset(h, more):
    h.reset(*((R,) if _runs(type(h)) else ()), K, N, CAP, *more)


def _append(h, run, block):
    h.append(run, block) if _runs(type(h)) else h.append(block)


def _shape(h):
    return (h.n_runs if _runs(type(h)) else None, h.n_clusters, h.n_objects, h.capacity)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


@pytest.mark.parametrize("cls,more,kept,word", STORES, ids=IDS)
def test_reset_hands_the_library_the_shape_and_the_units_trailing_argument(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch)
    tables = []

    def xlogx(n, made=partdist.xlogx):
        tables.append(made(n))
        return tables[-1]
    monkeypatch.setattr(partdist, "xlogx", xlogx)
    _reset(h, more)
    (name, args), = calls
    shape = (R, K, N, CAP) if _runs(cls) else (K, N, CAP)
    assert name == "reset" and args[1:1 + len(shape)] == shape and _shape(h) == ((R, K, N, CAP) if _runs(cls) else (None, K, N, CAP))
    behind = args[1 + len(shape):]
    if cls in (partdist.PartitionHandle, partsearch.SearchHandle):
        (table,) = tables
        assert behind == (_ptr(table),) and table.shape == (N + 1,)
    else:
        assert behind == more and tables == []
    if cls is simerr.SimErrHandle:
        assert h.batch_rows == 2
    assert h._stored == ([0] * R if _runs(cls) else 0)


@pytest.mark.parametrize("cls,more,kept,word", STORES, ids=IDS)
def test_an_append_that_fails_on_the_device_raises_the_librarys_message_and_unshapes_a_store_with_an_image(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch, append_code=2)
    _reset(h, more)
    with pytest.raises(_handle.EngineError, match="sbe error 2: refused"):
        _append(h, 1, _z(2, K, N))
    assert [name for name, _a in calls] == ["reset", "append_rows"]
    if cls is align.AlignHandle:                                # (no operand image: the shape stays)
        assert _shape(h) == (R, K, N, CAP) and h._stored == [0, 0]
    else:
        assert _shape(h) == ((0, 0, 0, 0) if _runs(cls) else (None, 0, 0, 0)) and h._stored == ([] if _runs(cls) else 0)
        if cls is simerr.SimErrHandle:
            assert h.batch_rows == 0


@pytest.mark.parametrize("cls,more,kept,word", STORES, ids=IDS)
def test_an_append_that_the_library_refuses_raises_and_leaves_the_shape_and_the_rows(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch, append_code=1)
    _reset(h, more)
    with pytest.raises(_handle.EngineError, match="sbe error 1: refused"):
        _append(h, 1, _z(2, K, N))
    assert _shape(h) == ((R, K, N, CAP) if _runs(cls) else (None, K, N, CAP)) and h._stored == ([0, 0] if _runs(cls) else 0)
    if cls is simerr.SimErrHandle:
        assert h.batch_rows == 2


@pytest.mark.parametrize("cls,more,kept,word", [c for c in STORES if c[2]], ids=[c[0].__name__ for c in STORES if c[2]])
def test_a_non_empty_append_marks_the_results_out_of_date_and_an_empty_one_does_not(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch)
    _reset(h, more)
    assert getattr(h, kept) == [0, 0]
    setattr(h, kept, [5, 6])
    h.append(0, _z(0, K, N))
    assert getattr(h, kept) == [5, 6] and h._stored == [0, 0]
    h.append(1, _z(2, K, N))
    assert getattr(h, kept) == [0, 0] and h._stored == [0, 2]
    assert [name for name, _a in calls] == ["reset", "append_rows", "append_rows"]


@pytest.mark.parametrize("cls,more,kept,word", RUN_STORES, ids=IDS[:4])
def test_the_mask_of_a_selection(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch)
    h.reset(3, K, N, CAP, *more)
    assert h._mask(None).tolist() == [1, 1, 1] and h._mask([2, 0, 2]).tolist() == [1, 0, 1] and h._mask([]).tolist() == [0, 0, 0]
    assert h._mask(range(1, 3)).dtype == np.uint8
    with pytest.raises(ValueError) as e:
        h._mask([0, 3])
    assert str(e.value) == "run 3 out of range [0, 3)"


def _question(h):
    """A call that asks something of the store."""
    return {align.AlignHandle: lambda: h.within(), consensus.ConsensusHandle: lambda: h.similarity(), partdist.PartitionHandle: lambda: h.sums(),
            simerr.SimErrHandle: lambda: h.moments(), partsearch.SearchHandle: lambda: h.evaluate(_z(1, N))}[type(h)]


@pytest.mark.parametrize("cls,more,kept,word", STORES, ids=IDS)
def test_the_refusals_before_any_library_call_read_the_same_for_every_class(monkeypatch, cls, more, kept, word):
    h, calls = _fake(cls, monkeypatch)

    def refused(call):
        with pytest.raises(ValueError) as e:
            call()
        return str(e.value)
    assert refused(_question(h)) == "the store has no shape yet (reset)"
    noun = cls._limits.noun if _runs(cls) else partsearch.LIMITS.noun
    if _runs(cls):
        assert refused(lambda: h.reset(65, K, N, CAP, *more)) == f"65 runs; {noun} takes 1 .. 64"
        assert refused(lambda: h.reset(R, 9, N, CAP, *more)) == f"9 clusters; {noun} takes 1 .. 8"
        assert refused(lambda: h.reset(R, K, N, 0, *more)) == "capacity=0 out of range [1, 1048576] (2^20 samples per run)"
    else:
        assert refused(lambda: h.reset(9, N, CAP)) == f"9 clusters; {noun} takes 1 .. 8"
        assert refused(lambda: h.reset(K, N, 0)) == "capacity=0 out of range [1, 65536] (2^16 samples)"
    assert calls == []
    _reset(h, more)
    if _runs(cls):
        for run in (-1, R):
            assert refused(lambda: h.append(run, _z(1, K, N))) == f"run {run} out of range [0, {R})"
        h._stored = [CAP - 1, 0]
        assert refused(lambda: h.append(0, _z(2, K, N))) == f"store overflow: run 0 holds {CAP - 1} samples, 2 more exceed the capacity of {CAP}"
    else:
        h._stored = CAP - 1
        assert refused(lambda: h.append(_z(2, K, N))) == f"store overflow: the store holds {CAP - 1} samples, 2 more exceed the capacity of {CAP}"
    assert refused(lambda: _append(h, 0, _z(1, K, N + 1))) == f"samples are {K} clusters x {N + 1} objects, the store holds {K} x {N}"
    assert refused(lambda: _append(h, 0, _z(N))) == f"cluster samples must be [n_samples, n_clusters, n_objects], got shape ({N},)"
    assert refused(lambda: _append(h, 0, np.full((1, K, N), 2, dtype=np.uint8))) == "cluster samples must hold 0 and 1 only"
    with pytest.raises(TypeError, match="boolean or integer 0 / 1, got float64"):
        _append(h, 0, np.zeros((1, K, N)))
    if word:
        method = getattr(h, {"slot": "similarity", "side": "moments"}[word])
        for index in (2, -1, True, 0.5):
            assert refused(lambda: method([0], **{word: index})) == f"{word}={index!r} is neither 0 nor 1"
    assert [name for name, _a in calls] == ["reset"]


def test_every_array_the_shared_layer_hands_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(_clusters)


# ---- the command lines' reader -------------------------------------------------------------------------------------------
def _files(folder, names, n_objects=None):
    folder.mkdir(parents=True, exist_ok=True)
    paths = []
    for i, name in enumerate(names):
        paths.append(folder / name)
        align.write_clusters(paths[-1], _z(2 + i, K, (n_objects or [5] * len(names))[i]))
    return [str(p) for p in paths]


def test_the_reader_takes_the_tag_and_the_run_names_from_the_file_names(tmp_path):
    ap = _clusters.runs_parser("prog", "what it does")
    args = ap.parse_args(_files(tmp_path / "in", ["clusters_K3_a.txt", "clusters_K3_run_b.txt"]))
    assert (args.burnin, args.out, args.device) == (0.0, None, None)
    runs, tag, names, out = _clusters.read_runs(args)
    assert [r.shape for r in runs] == [(2, K, 5), (3, K, 5)] and all(r.dtype == np.uint8 for r in runs)
    assert (tag, names, out) == ("K3", ["a", "run_b"], tmp_path / "in")


def test_the_reader_falls_back_to_the_samples_clusters_and_the_runs_numbers(tmp_path):
    args = _clusters.runs_parser("prog", "what it does").parse_args(_files(tmp_path, ["first.txt", "clusters_K3_b.txt", "clusters_b.txt"]))
    _runs_read, tag, names, _out = _clusters.read_runs(args)
    assert (tag, names) == (f"K{K}", ["0", "b", "2"])
    # the tag is the first file's: a name that says another K than the samples hold is taken at its word
    args = _clusters.runs_parser("prog", "what it does").parse_args(_files(tmp_path, ["clusters_K12_x.txt"]))
    assert _clusters.read_runs(args)[1:3] == ("K12", ["x"])


def test_the_reader_makes_the_output_folder_it_is_given(tmp_path):
    out = tmp_path / "deep" / "out"
    args = _clusters.runs_parser("prog", "what it does").parse_args(_files(tmp_path, ["clusters_K3_a.txt"]) + ["--out", str(out), "--burnin", "0.25", "--device", "1"])
    assert not out.exists() and (args.burnin, args.device) == (0.25, 1)
    assert _clusters.read_runs(args)[3] == out and out.is_dir()
    assert _clusters.read_runs(args)[3] == out                                         # (a folder that is there already)


def test_the_reader_ends_the_program_when_the_files_differ(tmp_path):
    out = tmp_path / "out"
    args = _clusters.runs_parser("prog", "what it does").parse_args(_files(tmp_path, ["clusters_K3_a.txt", "clusters_K3_b.txt"], [5, 6]) + ["--out", str(out)])
    with pytest.raises(SystemExit) as e:
        _clusters.read_runs(args)
    assert str(e.value) == f"the files differ in clusters or objects: [({K}, 5), ({K}, 6)]" and not out.exists()
