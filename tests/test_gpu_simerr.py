"""sbayes_amd.simerr on the device against the checker (tests/_simerr_oracle.py).  The moments are integers and z2 is formed
from exactly representable integers in a fixed order: every comparison is for equality, z2 included."""
import math

import numpy as np
import pytest

from sbayes_amd import align, consensus, simerr
from sbayes_amd._handle import EngineError
from tests import _simerr_cases as cases
from tests import _simerr_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = simerr.SimErrHandle()
    yield h
    h.close()


def fill(h, runs, b, capacity=None, pieces=None, n_runs=None, positions=None):
    """`runs` into a freshly shaped store of batches of b: optionally a larger store, rows appended in pieces of the sizes
    given (in turn, repeated), more runs in the store than given and the given ones at chosen positions."""
    k, n = runs[0].shape[1:]
    positions = list(range(len(runs))) if positions is None else positions
    h.reset(len(runs) if n_runs is None else n_runs, k, n, capacity or max(max(r.shape[0] for r in runs), b), b)
    for pos, run in zip(positions, runs):
        at, turn = 0, 0
        while at < run.shape[0]:
            size = pieces[turn % len(pieces)] if pieces else run.shape[0]
            h.append(pos, run[at:at + size])
            at, turn = at + size, turn + 1
        assert h.rows(pos) == run.shape[0]
    return positions


def check_moments(got, runs, b, what):
    s1, s2, nb = orc.moments(runs, b)
    assert got.s1.dtype == np.int32 and got.s2.dtype == np.int64 and got.s1.shape == got.s2.shape == s1.shape, what
    assert got.n_batches == nb, what
    for name, have, want in (("S1", got.s1, s1), ("S2", got.s2, s2)):
        bad = np.argwhere(have != want)
        assert bad.size == 0, f"{what}: {len(bad)} entries of {name} differ, first at {bad[0]}: device {have[tuple(bad[0])]}, checker {want[tuple(bad[0])]}"
    return s1, s2, nb


def check_compare(h, side_a, side_b, thresholds, what):
    got = h.compare(thresholds, z2=True)
    z, row_max, row_arg, row_count = orc.compare(side_a, side_b, thresholds)
    assert got.z2.dtype == got.row_max.dtype == np.float64 and got.row_arg.dtype == got.row_count.dtype == np.int32, what
    assert np.array_equal(got.z2, z), f"{what}: z2 differs at {np.argwhere(got.z2 != z)[:3].tolist()}"
    assert np.array_equal(got.row_max, row_max) and np.array_equal(got.row_arg, row_arg), what
    assert got.row_count.shape == (len(z), len(thresholds)) and np.array_equal(got.row_count, row_count), what
    lean = h.compare(thresholds)                                # without the matrix: the same rows
    assert lean.z2 is None and np.array_equal(lean.row_max, row_max) and np.array_equal(lean.row_arg, row_arg) and np.array_equal(lean.row_count, row_count)
    return z


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("k", cases.KS)
def test_moments_and_comparison_equal_the_checker_over_tile_edges_and_clusters(handle, k, n):
    b = 3
    runs = [cases.overlapping(2 * b + 1, k, n, seed=7600 + 10 * n + k, density=0.4), cases.disjoint(3 * b, k, n, seed=7601 + 10 * n + k)]
    fill(handle, runs, b)
    check_moments(handle.moments(), runs, b, f"K={k} N={n}, both runs")
    assert handle.last_kernel_ms() > 0.0 and handle.side_batches[0] == 5
    side_a = check_moments(handle.moments([0], side=0), runs[:1], b, f"K={k} N={n}, run 0")
    side_b = check_moments(handle.moments([1], side=1), runs[1:], b, f"K={k} N={n}, run 1")
    z = check_compare(handle, side_a, side_b, cases.THRESHOLDS, f"K={k} N={n}")
    assert np.array_equal(z, z.T) and handle.last_kernel_ms() > 0.0


@pytest.mark.parametrize("b,k", cases.BATCH_SHAPES)
def test_batches_below_at_and_above_whole_steps_and_rounds(handle, b, k):
    assert b * k in (1, 63, 64, 65, 128, 257, 320, 560)
    runs = [cases.overlapping(s, k, 33, seed=7700 + b + k + s, density=0.45) for s in (2 * b, 3 * b + min(b - 1, 2))]
    fill(handle, runs, b)
    check_moments(handle.moments(), runs, b, f"b={b} K={k}")
    side_a = check_moments(handle.moments([0], side=0, copy=True), runs[:1], b, f"b={b} K={k}, run 0")
    side_b = check_moments(handle.moments([1], side=1, copy=True), runs[1:], b, f"b={b} K={k}, run 1")
    check_compare(handle, side_a, side_b, (3.84,), f"b={b} K={k}")


def test_run_lengths_a_trailing_batch_ignored_then_completed_and_sides_of_several_runs(handle):
    b, k, n = 5, 3, 33
    full = [cases.overlapping(s, k, n, seed=7800 + s) for s in (3 * b, b - 1, b, 2 * b, 2 * b + 1)]
    at = fill(handle, full, b, n_runs=6, positions=[4, 0, 5, 2, 1], capacity=4 * b, pieces=[3, 4])
    for runs, what in [([3], "S = 2 b"), ([4], "S = 2 b + 1: the trailing sample is not used"), ([1, 3], "S = b - 1 (no batch) beside S = 2 b"),
                       ([0, 3], "two runs of different lengths"), ([0, 2, 4], "three runs of different lengths"), ([0, 1, 2, 3, 4], "every run")]:
        got = handle.moments([at[r] for r in runs] + [3])        # (run 3 of the store is empty)
        check_moments(got, [full[r] for r in runs], b, what)
    for runs, counts in [([1], "0 complete batches of 5 rows (4 rows in all)"), ([2], "1 complete batches of 5 rows (5 rows in all)"),
                         ([1, 2], "1 complete batches of 5 rows (9 rows in all)")]:
        mask = np.zeros(6, dtype=np.uint8)
        mask[[at[r] for r in runs]] = 1
        assert handle._lib.sbe_simerr_moments(handle._h, mask.ctypes.data, 0, None, None, None) == 3, runs      # SBE_ERR_STATE
        assert counts in handle._last_error() and "at least 2" in handle._last_error()
    # later appends complete the trailing batches: S = 2 b + 1 becomes 3 b, S = b - 1 becomes b + 1
    rest = cases.overlapping(b - 1, k, n, seed=7810)
    grown = np.concatenate([full[4], rest])
    handle.append(at[4], rest[:1])
    handle.append(at[4], rest[1:])
    two = cases.overlapping(2, k, n, seed=7811)
    handle.append(at[1], two)
    check_moments(handle.moments([at[4]]), [grown], b, "S = 3 b after the append")
    assert handle.side_batches[0] == 3
    check_moments(handle.moments([at[1], at[2]]), [np.concatenate([full[1], two]), full[2]], b, "S = b + 1 and S = b")


@pytest.mark.parametrize("b,k", [(7, 3), (13, 5), (3, 1), (16, 8)])
def test_pieces_that_split_inside_a_batch_a_step_and_a_dword(handle, b, k):
    s = 4 * b + 2
    c = cases.overlapping(s, k, 70, seed=7900 + 10 * b + k)
    fill(handle, [c], b)
    whole = handle.moments()
    check_moments(whole, [c], b, f"b={b} K={k}, one piece")
    fill(handle, [c], b, pieces=[1])                            # one sample at a time
    single = handle.moments()
    assert np.array_equal(single.s1, whole.s1) and np.array_equal(single.s2, whole.s2) and single.n_batches == whole.n_batches == 4
    for pieces in ([b - 1, 2, b + 3], [3, 5, 1, 2], [2 * b + 1]):
        assert any((p * k) % 8 for p in pieces) or k == 8
        fill(handle, [c], b, pieces=pieces, capacity=6 * b + 5)  # a store larger than its rows
        mixed = handle.moments()
        assert np.array_equal(mixed.s1, whole.s1) and np.array_equal(mixed.s2, whole.s2), pieces


def test_one_launch_and_one_tile_pair_per_launch_give_the_same_bits(handle):
    b = 4
    runs = [cases.overlapping(13, 8, 257, seed=8000), cases.overlapping(9, 8, 257, seed=8001)]      # 9 tiles, 45 tile pairs
    fill(handle, runs, b)
    try:
        handle.set_launch_tiles(0)
        whole = handle.moments()
        for tiles in (1, 7):
            handle.set_launch_tiles(tiles)
            got = handle.moments(side=1)
            assert np.array_equal(got.s1, whole.s1) and np.array_equal(got.s2, whole.s2), tiles
        with pytest.raises(EngineError, match="tile_pairs=-1 out of range"):
            handle.set_launch_tiles(-1)
    finally:
        handle.set_launch_tiles(0)
    check_moments(whole, runs, b, "K=8 N=257")
    same = handle.compare((0.0,))                               # both sides hold the same moments
    assert not same.row_max.any() and not same.row_arg.any() and not same.row_count.any()


def test_both_triangles_are_filled_and_the_diagonal_tiles_are_right(handle):
    # objects in ascending blocks: an asymmetric error (a tile written at its mirror's place, rows for columns) would show
    n, b = 100, 2
    c = np.zeros((6, 4, n), dtype=np.uint8)
    for s in range(6):
        for k in range(4):
            c[s, k, 7 * k + s: 7 * k + s + 10 + 9 * k] = 1
    fill(handle, [c], b)
    got = handle.moments()
    s1, s2, _nb = check_moments(got, [c], b, "ascending blocks")
    assert np.array_equal(got.s1, got.s1.T) and np.array_equal(got.s2, got.s2.T)
    assert not np.array_equal(s1[:32, 32:64], s1[:32, 32:64].T)             # (an off-diagonal tile is not symmetric in itself)
    assert np.array_equal(np.diag(got.s1), c.sum(axis=(0, 1)))


def test_s1_equals_the_consensus_counts_when_the_batch_divides_every_run(handle):
    b = 6
    runs = [cases.overlapping(s, 5, 65, seed=8100 + s) for s in (4 * b, 2 * b, 7 * b)]
    fill(handle, runs, b)
    hc = consensus.ConsensusHandle()
    try:
        hc.reset(3, 5, 65, 7 * b)
        for r, run in enumerate(runs):
            hc.append(r, run)
        for sel in (None, [0, 2], [1]):
            got = handle.moments(sel)
            assert np.array_equal(got.s1, hc.similarity(sel)) and got.n_batches * b == hc.slot_samples[0]
    finally:
        hc.close()


def test_the_limit_of_the_accumulator_two_runs_of_2_to_the_20_rows():
    rows = cases.limit_run()                                                # 16 MiB of host rows per run
    b = 1 << 10
    h = simerr.SimErrHandle()
    try:
        h.reset(3, 8, 2, 1 << 20, b)
        h.append(0, rows)
        h.append(1, rows[:(1 << 19) + 5])                                   # (the piece ends inside a batch)
        h.append(1, rows[(1 << 19) + 5:])
        for sel, n_runs in (([0, 1], 2), ([1], 1)):
            got = h.moments(sel)
            s1, s2, nb = cases.limit_moments(n_runs)
            assert got.n_batches == nb == n_runs << 10 and got.s1.tolist() == s1 and got.s2.tolist() == s2, sel
            assert got.variance.tolist() == [[nb * s2[i][j] - s1[i][j] ** 2 for j in range(2)] for i in range(2)]
        assert got.variance[0, 0] == 0 and got.variance[0, 1] > 0 and h.moments([0, 1]).s1[0, 0] == 1 << 24
        h.append(2, rows[:b])                                               # T K = 2^24 + b K: refused by the library itself
        mask = np.ones(3, dtype=np.uint8)
        assert h._lib.sbe_simerr_moments(h._h, mask.ctypes.data, 0, None, None, None) == 1
        assert "2098176 rows x 8 clusters = 16785408 elements, the limit is 16777216" in h._last_error()
        with pytest.raises(ValueError, match="16785408 elements"):
            h.moments()
    finally:
        h.close()


def test_thresholds_from_none_to_four_and_strictly_above_an_attained_value(handle):
    b = 4
    runs = [cases.disjoint(6 * b, 3, 40, seed=8200), cases.disjoint(5 * b, 3, 40, seed=8201)]
    fill(handle, runs, b)
    side_a = check_moments(handle.moments([0], side=0), runs[:1], b, "run 0")
    side_b = check_moments(handle.moments([1], side=1), runs[1:], b, "run 1")
    z = orc.z2(side_a, side_b)
    attained = sorted(set(z[np.isfinite(z) & (z > 0)].tolist()))
    assert len(attained) > 8
    low, mid = attained[1], attained[len(attained) // 2]
    for thresholds in ((), (mid,), (low, mid), (mid, low, 0.0), (math.inf, -1.0, mid, math.nextafter(mid, 0.0))):
        check_compare(handle, side_a, side_b, thresholds, f"{len(thresholds)} thresholds")
    got = handle.compare((mid, math.nextafter(mid, 0.0)))
    assert int(got.row_count[:, 1].sum()) - int(got.row_count[:, 0].sum()) == int((z == mid).sum()) > 0      # strictly above
    assert handle._lib.sbe_simerr_compare(handle._h, None, 5, None, got.row_max.ctypes.data, got.row_arg.ctypes.data, None) == 1
    assert "n_thresholds=5 out of range [0, 4]" in handle._last_error()
    bad = np.array([1.0, math.nan])
    assert handle._lib.sbe_simerr_compare(handle._h, bad.ctypes.data, 2, None, got.row_max.ctypes.data, got.row_arg.ctypes.data, got.row_count.ctypes.data) == 1
    assert "thresholds[1] is not a number" in handle._last_error()


def test_the_planted_degenerate_cases(handle):
    b, nb = 4, 3
    runs = cases.planted(b, nb)
    fill(handle, runs, b)
    side_a = check_moments(handle.moments([0], side=0), runs[:1], b, "run a")
    side_b = check_moments(handle.moments([1], side=1), runs[1:], b, "run b")
    check_compare(handle, side_a, side_b, (0.0, math.inf), "planted")
    got = handle.compare((0.0, math.inf), z2=True)
    assert got.z2[0, 1] == 0.0 and got.z2[0, 2] == got.z2[0, 8] == math.inf and got.row_max[0] == math.inf and got.row_arg[0] == 2
    assert not got.z2[3].any() and got.row_arg[3] == 0 and got.row_count[3].tolist() == [0, 0] and got.z2[4, 7] == 1.0
    assert not got.row_count[:, 1].any() and np.array_equal(got.z2[:, 5], got.z2[:, 6])


def test_state_errors_and_what_the_library_refuses_itself(handle):
    h = handle
    c = cases.overlapping(9, 3, 10, seed=8300)
    for args, text in [((1, 9, 10, 4, 2), "n_clusters=9"), ((1, 8, 8193, 4, 2), "n_objects=8193 out of range [1, 8192]"), ((65, 2, 10, 4, 2), "n_runs=65"),
                       ((1, 2, 10, (1 << 20) + 1, 2), "capacity_rows"), ((1, 2, 10, 4, 0), "batch_rows=0 out of range [1, 4]"),
                       ((1, 2, 10, 4, 5), "batch_rows=5 out of range [1, 4]"), ((1, 1, 8192, 1 << 20, 1), "the limit is 17179869184")]:
        assert h._lib.sbe_simerr_reset(h._h, *args) == 1 and text in h._last_error(), text
    h.reset(3, 3, 10, 12, 2)
    mask = np.ones(3, dtype=np.uint8)
    assert h._lib.sbe_simerr_moments(h._h, mask.ctypes.data, 0, None, None, None) == 3                 # a selection without rows
    assert "0 complete batches of 2 rows (0 rows in all)" in h._last_error()
    assert h._lib.sbe_simerr_moments(h._h, mask.ctypes.data, 2, None, None, None) == 1 and "side=2" in h._last_error()
    assert h._lib.sbe_simerr_moments(h._h, None, 0, None, None, None) == 1 and "run_mask" in h._last_error()
    bad = c.copy()
    bad[3, 2, 7] = 2
    assert h._lib.sbe_simerr_append_rows(h._h, 0, bad.ctypes.data, 5) == 4 and "rows[3][2][7]=2 is neither 0 nor 1" in h._last_error()
    assert h.rows(0) == 0
    assert h._lib.sbe_simerr_append_rows(h._h, 0, np.zeros((13, 3, 10), dtype=np.uint8).ctypes.data, 13) == 1 and "store overflow" in h._last_error()
    assert h._lib.sbe_simerr_append_rows(h._h, 3, c.ctypes.data, 1) == 1 and "run 3 out of range" in h._last_error()
    assert h._lib.sbe_simerr_append_rows(h._h, 0, None, 1) == 1 and "null pointer" in h._last_error()
    h.append(0, c)
    h.append(1, c[:5])
    with pytest.raises(EngineError, match="side 0 is empty") as err:
        h.compare()
    assert err.value.code == 3
    h.moments([0], side=0, copy=False)
    with pytest.raises(EngineError, match="side 1 is empty"):
        h.compare()
    assert h.moments([1], side=1, copy=False).s1 is None and h.side_batches == [4, 2]
    h.compare()
    h.append(2, c[:4])                                                                          # the store changes
    assert h.side_batches == [0, 0]
    with pytest.raises(EngineError, match="side 0 was computed before the store last changed") as err:
        h.compare()
    assert err.value.code == 3
    h.moments([0], side=0, copy=False)                                                           # a side recomputed: the other one is stale
    with pytest.raises(EngineError, match="side 1 was computed before the store last changed"):
        h.compare()
    h.moments([2], side=1, copy=False)
    assert np.array_equal(h.compare(z2=True).z2, orc.z2(orc.moments([c], 2), orc.moments([c[:4]], 2)))
    out = np.zeros(10)
    ints = np.zeros(10, dtype=np.int32)
    assert h._lib.sbe_simerr_compare(h._h, None, 0, None, None, ints.ctypes.data, None) == 1 and "row_max" in h._last_error()
    assert h._lib.sbe_simerr_compare(h._h, None, 0, None, out.ctypes.data, None, None) == 1 and "row_arg" in h._last_error()
    assert h._lib.sbe_simerr_compare(h._h, None, 1, None, out.ctypes.data, ints.ctypes.data, ints.ctypes.data) == 1 and "thresholds" in h._last_error()
    assert h._lib.sbe_simerr_compare(h._h, out.ctypes.data, 1, None, out.ctypes.data, ints.ctypes.data, None) == 1 and "row_count" in h._last_error()
    fresh = simerr.SimErrHandle()
    try:
        with pytest.raises(EngineError, match="no shape yet"):
            fresh._check(fresh._lib.sbe_simerr_moments(fresh._h, mask.ctypes.data, 0, None, None, None))
    finally:
        fresh.close()


def test_the_one_call_functions_on_the_recorded_runs():
    runs = cases.diag_runs()
    assert [r.shape[0] for r in runs] == [60, 60]
    b = orc.default_batch_rows(runs, 0.1)
    kept = orc.trim(runs, 0.1, b)
    assert b == 7 and [len(r) for r in kept] == [49, 49]                    # 54 samples after burn-in, floor(sqrt(54)) = 7
    err = simerr.similarity_error(runs, burnin=0.1)
    s1, s2, nb = orc.moments(kept, b)
    assert (err.n_batches, err.batch_rows, err.n_samples) == (nb, b, 98) and err.counts.dtype == np.int32
    assert np.array_equal(err.counts, s1) and np.array_equal(err.variance, orc.variance(s1, s2, nb))
    assert np.array_equal(err.probability, orc.probability(s1, nb, b)) and np.array_equal(err.se, np.sqrt(orc.se_squared(s1, s2, nb, b)))
    assert err.se.any() and np.isinf(err.ess[err.se == 0]).all() and err.kernel_ms > 0.0
    assert np.array_equal(simerr.similarity_error(runs, burnin=0.1, batch_rows=9).counts, orc.moments(orc.trim(runs, 0.1, 9), 9)[0])
    agr = simerr.run_agreement(runs + [runs[0][5:]], burnin=0.1, batch_rows=6)
    three = orc.trim(runs + [runs[0][5:]], 0.1, 6)
    want = orc.run_agreement(three, 6, cases.THRESHOLDS)
    assert agr.n_batches == (9, 9, 8) and agr.batch_rows == 6 and agr.thresholds == cases.THRESHOLDS
    for (a, c), (best, pair, shares, max_abs, object_max) in want.items():
        for p, q in ((a, c), (c, a)):
            assert agr.max_z2[p, q] == best and tuple(agr.pair[p, q]) == pair and agr.share[p, q].tolist() == shares, (p, q)
            assert agr.max_abs[p, q] == max_abs and np.array_equal(agr.object_max[p, q], object_max), (p, q)
    assert not np.diag(agr.max_z2).any() and agr.max_z2[0, 1] > 0.0
    cmp = consensus.compare_runs([three[0], three[1]])
    assert agr.max_abs[0, 1] == cmp.max_abs[0, 1]                           # (6 divides both lengths: the same samples)


def test_command_line_writes_the_standard_errors_and_the_agreement(tmp_path, capsys):
    runs = cases.diag_runs()
    files = []
    for r, run in enumerate(runs):
        files.append(tmp_path / f"clusters_K3_{r}.txt")
        align.write_clusters(files[-1], run)
    out = tmp_path / "summary"
    assert simerr.main([str(f) for f in files] + ["--burnin", "0.1", "--batch", "6", "--out", str(out)]) == 0
    text = capsys.readouterr().out
    kept = orc.trim(runs, 0.1, 6)
    s1, s2, nb = orc.moments(kept, 6)
    assert nb == 18 and "108 samples in 18 batches of 6 after burn-in" in text
    assert np.array_equal(consensus.read_similarity(out / "similarity_se_K3.txt"), np.sqrt(orc.se_squared(s1, s2, nb, 6)))
    best, pair, shares, max_abs, _rows = orc.run_agreement(kept, 6, cases.THRESHOLDS)[0, 1]
    lines = (out / "agreement_K3.tsv").read_text().splitlines()
    assert len(lines) == 2 and lines[0].startswith("run_a\trun_b\tbatches_a\tbatches_b\tbatch_rows\tmax_z2")
    assert lines[1].split("\t") == ["clusters_K3_0.txt", "clusters_K3_1.txt", "9", "9", "6", repr(float(best)), str(pair[0]), str(pair[1]), repr(max_abs)] + [repr(s) for s in shares]
