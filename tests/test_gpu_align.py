"""sbayes_amd.align on the device against the checker (tests/_align_oracle.py).  Permutations, counts and agreements are
integers: every comparison is for equality."""
from itertools import permutations
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import align, diag
from sbayes_amd._handle import EngineError
from tests import _align_cases as cases
from tests import _align_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
KS, NS, LENGTHS = (1, 2, 5, 8), (1, 31, 32, 33, 64, 257), (1, 2, 19, 20, 21, 48)


def device_within(runs, seed, capacity=None, pieces=None, n_runs=None, positions=None):
    """Permutations of `runs` from one handle: optionally a larger store, rows appended in pieces, more runs in the handle
    than given and the given ones at chosen positions."""
    k, n = runs[0].shape[1:]
    n_runs = len(runs) if n_runs is None else n_runs
    positions = list(range(len(runs))) if positions is None else positions
    h = align.AlignHandle()
    try:
        h.reset(n_runs, k, n, capacity or max(max(r.shape[0] for r in runs), 1))
        for pos, run in zip(positions, runs):
            at = 0
            for size in (pieces or [run.shape[0]]):
                h.append(pos, run[at:at + size])
                at += size
            if at < run.shape[0]:
                h.append(pos, run[at:])
            assert h.rows(pos) == run.shape[0]
        perms = h.within(seed)
        assert h.last_kernel_ms() > 0.0
        return [perms[pos] for pos in positions]
    finally:
        h.close()


def check_within(c, seed, what):
    got = device_within([c], seed)[0]
    want = orc.within(c, seed)
    assert got.dtype == np.int8 and got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}, seed {seed}: first differing step {bad[0]}: device {got[bad[0]]}, checker {want[bad[0]]}"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_within_run_equals_the_checker_over_cluster_and_word_edges(k, n):
    c, _ = cases.planted(k, n, seed=3000 + 10 * n + k)
    for seed in (0, 20):
        check_within(c, seed, f"K={k} N={n}")


@pytest.mark.parametrize("s", LENGTHS)
def test_within_run_at_the_edges_of_the_seed_window(s):
    c, _ = cases.planted(5, 100, s, seed=3100 + s)
    for seed in (0, 20, 1024):
        check_within(c, seed, f"S={s}")


def test_a_lane_owns_more_than_one_word():
    n = 8192 + 65                                                           # 259 words for 256 lanes
    assert n <= align.max_objects(2)
    c, _ = cases.planted(2, n, 12, seed=3200)
    for seed in (0, 5):
        check_within(c, seed, f"N={n}")


def test_the_largest_store_of_eight_clusters_and_one_object_more():
    n = align.max_objects(8)
    c, _ = cases.planted(8, n, 10, seed=3300)
    check_within(c, 3, f"K=8 N={n}")
    with pytest.raises(ValueError, match=f"{n + 1} objects"):
        align.match_online(np.zeros((2, 8, n + 1), dtype=np.uint8))
    h = align.AlignHandle()
    try:                                                                    # ... and by the library itself
        assert h._lib.sbe_align_reset(h._h, 1, 8, n + 1, 4) == 1
        assert f"n_objects={n + 1} out of range [1, {n}]" in h._last_error()
        assert h._lib.sbe_align_reset(h._h, 1, 9, 10, 4) == 1 and "n_clusters=9" in h._last_error()
        assert h._lib.sbe_align_reset(h._h, 65, 2, 10, 4) == 1 and "n_runs=65" in h._last_error()
        assert h._lib.sbe_align_reset(h._h, 1, 2, 10, (1 << 20) + 1) == 1 and "capacity_rows" in h._last_error()
        h.reset(2, 2, 10, 4)
        rows = np.zeros((5, 2, 10), dtype=np.uint8)
        assert h._lib.sbe_align_append_rows(h._h, 0, rows.ctypes.data, 5) == 1 and "store overflow" in h._last_error()
        assert h._lib.sbe_align_append_rows(h._h, 2, rows.ctypes.data, 1) == 1 and "run 2 out of range" in h._last_error()
        assert h._lib.sbe_align_append_rows(h._h, 0, None, 1) == 1 and "null pointer" in h._last_error()
        assert h._lib.sbe_align_within(h._h, 1025, rows.ctypes.data) == 1 and "seed_rows=1025" in h._last_error()
        assert h._lib.sbe_align_within(h._h, 0, None) == 1 and "null pointer" in h._last_error()
        h.append(0, rows[:3])
        with pytest.raises(EngineError, match="sbe_align_within comes first"):
            h.counts(aligned=True)
        with pytest.raises(EngineError, match=r"burn_rows\[0\]=4 out of range \[0, 3\]"):
            h.counts(aligned=False, burn_rows=[4, 0])
        assert h.counts(aligned=False).shape == (2, 2, 10)
    finally:
        h.close()


@pytest.mark.parametrize("n_runs", [1, 3, 64])
def test_runs_of_unequal_lengths_go_in_parallel(n_runs):
    rng = np.random.default_rng(3400 + n_runs)
    lengths = [48] + [int(v) for v in rng.integers(1, 48, n_runs - 1)]
    runs = [cases.planted(3, 40, s, seed=3500 + 7 * r)[0] for r, s in enumerate(lengths)]
    for seed in (0, 20):
        got = device_within(runs, seed)
        for r, run in enumerate(runs):
            assert np.array_equal(got[r], orc.within(run, seed)), f"run {r} of {n_runs}, seed {seed}"


@pytest.mark.parametrize("name", sorted(cases.tie_cases()))
def test_under_ties_the_device_takes_the_smallest_maximiser(name):
    c = cases.tie_cases()[name]
    _p, ds = orc.within(c, 0, with_d=True)
    assert sum(orc.count_optimal(d) > 1 for d in ds) > 1                    # ties beyond the first step
    for seed in (0, 20):
        check_within(c, seed, name)


@pytest.mark.parametrize("k,n", [(2, 33), (5, 100), (6, 70)])
def test_every_device_permutation_is_optimal_for_the_matrix_it_saw(k, n):
    """Independent of the checker's solver: d is rebuilt from the device's own earlier permutations and the maximum is
    found by a plain loop over all permutations."""
    c, _ = cases.planted(k, n, flip=0.15, seed=3600 + k)
    for seed in (0, 20):
        got = device_within([c], seed)[0].astype(np.int64)
        m = min(seed, c.shape[0])
        total = c[:m].astype(np.int64).sum(axis=0)
        for s in range(c.shape[0]):
            assert sorted(got[s]) == list(range(k))
            d = total @ c[s].astype(np.int64).T
            best = max(sum(int(d[i, p[i]]) for i in range(k)) for p in permutations(range(k)))
            assert int(d[np.arange(k), got[s]].sum()) == best, f"step {s}"
            total += max(m, 1) * c[s][got[s]]


def test_bits_do_not_depend_on_appends_capacity_position_or_company():
    c, _ = cases.planted(5, 100, seed=3700)
    other, _ = cases.planted(5, 100, 31, seed=3701)
    for seed in (0, 20):
        base = device_within([c], seed)[0]
        assert np.array_equal(base, orc.within(c, seed))
        assert np.array_equal(device_within([c], seed, pieces=[1] * 48)[0], base)
        assert np.array_equal(device_within([c], seed, pieces=[5, 1, 17, 2])[0], base)
        assert np.array_equal(device_within([c], seed, capacity=1000)[0], base)
        got = device_within([other, c], seed, n_runs=7, positions=[2, 6], capacity=77)
        assert np.array_equal(got[1], base) and np.array_equal(got[0], orc.within(other, seed))


def test_long_rows_go_through_the_staging_buffer_in_pieces_at_any_offset():
    """At K = 2 and the most objects the store takes a sample is close to 40 KB, so the 64 MiB staging buffer holds about
    1 600 of them: 2 pieces + 3 samples appended in one call go in three pieces, and batches of piece - 1, 1, piece + 1, 4
    straddle the pieces at offsets that are not 0 (the run ends 2 samples into the last batch, which holds what is left).
    The counts as stored are the column sums of the host array, and both stores give the same permutations."""
    k, n = 2, align.max_objects(2)
    piece = (64 << 20) // (k * n)
    s = 2 * piece + 3
    c = np.random.default_rng(3600).integers(0, 2, (s, k, n), dtype=np.uint8)
    perms = []
    for batches in ((s,), (piece - 1, 1, piece + 1, 4)):
        h = align.AlignHandle()
        try:
            h.reset(1, k, n, s)
            at = 0
            for size in batches:
                h.append(0, c[at:at + size])
                at += size
            assert at >= s and h.rows(0) == s
            assert np.array_equal(h.counts(aligned=False)[0], c.sum(axis=0, dtype=np.int32))
            perms.append(h.within()[0])
        finally:
            h.close()
    assert perms[0].shape == (s, k) and np.array_equal(perms[0], perms[1])


def test_counts_aligned_and_as_logged_with_and_without_burn_in():
    lengths = [48, 20, 33]
    runs = [cases.planted(4, 65, s, seed=3800 + r)[0] for r, s in enumerate(lengths)]
    h = align.AlignHandle()
    try:
        h.reset(3, 4, 65, 50)
        for r, run in enumerate(runs):
            h.append(r, run)
        perms = h.within(20)
        for burn in ([0, 0, 0], [5, 20, 1]):
            aligned, logged = h.counts(True, burn), h.counts(False, burn)
            assert aligned.dtype == np.int32
            for r, run in enumerate(runs):
                assert np.array_equal(aligned[r], orc.counts(run, orc.within(run, 20), burn[r]))
                assert np.array_equal(logged[r], orc.counts(run, None, burn[r]))
                assert np.array_equal(perms[r], orc.within(run, 20))
        assert not aligned[1].any() and not np.array_equal(h.counts(True), h.counts(False))
    finally:
        h.close()


@pytest.mark.parametrize("within", [None, 0, 20])
def test_planted_relabellings_across_three_runs_are_recovered(within):
    k, n = 4, 100
    relabel = [[0, 1, 2, 3], [3, 1, 0, 2], [1, 2, 3, 0]]
    runs = cases.relabelled_runs(k, n, [40, 33, 48], relabel, seed=900, switch_every=0 if within is None else 5)
    for pivot in (0, 2):
        res = align.align_runs(runs, pivot=pivot, within=within, burnin=0.1)
        want = orc.align_runs(runs, pivot=pivot, within_seed=within, burnin=0.1)
        assert np.array_equal(res.run_perms, want["run_perms"]) and res.run_perms.dtype == np.int8
        assert np.array_equal(res.run_perms[pivot], np.arange(k))           # the pivot keeps its labels
        assert np.array_equal(res.agreement, want["agreement"]) and res.agreement.dtype == np.int64
        assert np.array_equal(res.counts, want["counts"])
        assert res.burn_rows == tuple(want["burn_rows"]) == (4, 3, 4)
        for r in range(3):
            assert np.array_equal(res.perms[r], want["perms"][r])
            assert np.array_equal(res.total_perms[r], want["total_perms"][r])
            assert np.array_equal(res.frequencies[r], res.counts[r] / (runs[r].shape[0] - res.burn_rows[r]))
            assert res.agreement_after(r) >= res.agreement_before(r)
        blocks = [cases.dominant_blocks(k, n, cnt) for cnt in res.counts]
        assert len(set(blocks[0])) == k and all(np.array_equal(b, blocks[0]) for b in blocks)
        if within is None:
            for r in range(3):
                assert np.array_equal(np.asarray(relabel[r])[res.run_perms[r]], relabel[pivot])


def _unpack(g, key, shape_key):
    s, k, n = (int(v) for v in g[shape_key])
    return np.unpackbits(g[key], axis=-1)[:, :, :n].reshape(s, k, n)


def _diag_runs():
    g = np.load(GOLDEN / "diag_runs.npz")
    kn = int(g["n_cluster_columns"])
    k = 1 + int(str(g["cluster_names"][-1]).split("_")[0][1:])
    return [np.unpackbits(g[f"clusters_{r}"], axis=1)[:, :kn].reshape(-1, k, kn // k) for r in range(2)], g


def test_what_the_reference_recorded_is_reproduced():
    g = np.load(GOLDEN / "align.npz")
    excluded = 0
    for tag in ("k3_n100", "k5_n33", "k7_n257"):
        c = _unpack(g, f"logger_{tag}_in", f"logger_{tag}_shape")
        got = align.match_online(c)
        unique = g[f"logger_{tag}_nopt"] == 1
        ds = orc.within(c, 0, with_d=True)[1]
        excluded += sum(1 for s in range(len(c)) if not unique[s] and ds[s].any())
        assert np.array_equal(got[unique], g[f"logger_{tag}_perms"][unique])
        assert np.array_equal(got[~unique], g[f"logger_{tag}_perms"][~unique])      # all-zero steps: the identity under both
        assert not unique[0] and np.array_equal(got[0], np.arange(c.shape[1]))
    for tag in ("k3_n100", "k5_n33"):
        c = _unpack(g, f"realign_{tag}_in", f"realign_{tag}_shape")
        excluded += int(np.count_nonzero(g[f"realign_{tag}_nopt"] != 1))
        perms = align.realign_within_run(c, seed=20)
        assert np.array_equal(align.apply(c, perms), _unpack(g, f"realign_{tag}_out", f"realign_{tag}_shape"))
        names = [str(v) for v in g[f"realign_{tag}_names"]]
        assert np.array_equal(align.permute_stats(names, g[f"realign_{tag}_params_in"], perms)[1], g[f"realign_{tag}_params_out"])
    runs, _ = _diag_runs()
    excluded += int(g["runs_diag_nopt"] != 1) + int(g["runs_planted_nopt"] != 1)
    assert np.array_equal(align.align_runs(runs).run_perms[1], g["runs_diag_perm"])
    n2 = int(g["runs_planted_shape"][1])
    planted = [np.unpackbits(g[f"runs_planted_in{r}"], axis=-1)[:, :, :n2] for r in range(2)]
    assert np.array_equal(align.align_runs(planted).run_perms[1], g["runs_planted_perm"])
    assert excluded == 0


def test_swapped_labels_are_undone_before_the_convergence_diagnostics():
    """The two recorded south_america runs.  As logged their labels do not correspond (the reference's align_clusters.py
    moves run 1 by the recorded permutation), so the pair with corresponding labels is (run 0, run 1 moved by it).  With
    the labels of run 1 swapped on purpose, and also as logged, align_runs gives back exactly that pair, hence its R-hat
    bit for bit; without alignment at least one indicator column has a larger R-hat."""
    runs, _ = _diag_runs()
    recorded = np.load(GOLDEN / "align.npz")["runs_diag_perm"].astype(np.intp)
    pair = [runs[0], runs[1][:, recorded]]
    swapped = [pair[0], np.ascontiguousarray(pair[1][:, [1, 0, 2]])]
    flat = lambda rs: [r.reshape(r.shape[0], -1).astype(np.float64) for r in rs]      # noqa: E731
    want = diag.convergence(flat(pair), burnin=0.1)
    for given in (swapped, runs):
        res = align.align_runs(given, pivot=0)
        aligned = [align.apply(r, p) for r, p in zip(given, res.total_perms)]
        assert np.array_equal(aligned[0], pair[0]) and np.array_equal(aligned[1], pair[1])
        got = diag.convergence(flat(aligned), burnin=0.1)
        assert np.array_equal(got.rhat, want.rhat, equal_nan=True) and np.array_equal(got.ess, want.ess, equal_nan=True)
    assert np.array_equal(align.align_runs(swapped).run_perms[1], [1, 0, 2])
    raw = diag.convergence(flat(swapped), burnin=0.1)
    both = np.isfinite(raw.rhat) & np.isfinite(want.rhat)
    assert (raw.rhat[both] > want.rhat[both]).any()


def test_command_line_writes_the_aligned_files(tmp_path, capsys):
    k, n = 3, 37
    relabel = [[0, 1, 2], [2, 0, 1]]
    runs = cases.relabelled_runs(k, n, [30, 26], relabel, seed=950, switch_every=4)
    folder = tmp_path / f"K{k}"
    folder.mkdir()
    header = ["Sample", "posterior"] + [f"size_a{i}" for i in range(k)] + ["w_areal_F1"] + [f"areal_a{i}_F1_x" for i in range(k)]
    tables = []
    for r, run in enumerate(runs):
        align.write_clusters(folder / f"clusters_K{k}_{r}.txt", run)
        table = np.column_stack([np.arange(len(run)) * 10.0, -100.0 - np.arange(len(run)), run.sum(axis=2),
                                 np.full(len(run), 0.25), 0.5 + 10 * np.arange(k)[None, :] + 100 * np.arange(len(run))[:, None]])
        with open(folder / f"stats_K{k}_{r}.txt", "w") as f:
            f.write("\t".join(header) + "\n")
            for row in table:
                f.write("\t".join("%.8g" % v for v in row) + "\n")
        tables.append(table)
    assert align.main(["-k", str(k), str(tmp_path), "0", "1", "--within", "20", "--pivot", "0"]) == 0
    text = capsys.readouterr().out
    want = orc.align_runs(runs, pivot=0, within_seed=20)
    for r, run in enumerate(runs):
        assert f"run {r}: permutation {want['run_perms'][r].tolist()}" in text
        aligned = align.read_clusters(folder / f"clusters_K{k}_{r}.aligned.txt")
        assert np.array_equal(aligned, align.apply(run, want["total_perms"][r]))
        names, rows = diag.read_stats(folder / f"stats_K{k}_{r}.aligned.txt")
        assert names == header
        assert np.array_equal(rows, align.permute_stats(header, tables[r], want["total_perms"][r])[1])
        assert np.array_equal(rows[:, 2:2 + k], aligned.sum(axis=2))         # the sizes moved with the clusters
    assert "agreement with the pivot" in text and (want["total_perms"][1] != np.arange(k)).any()
