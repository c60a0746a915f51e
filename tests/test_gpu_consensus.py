"""sbayes_amd.consensus on the device against the checker (tests/_consensus_oracle.py).  Counts, scores and the comparison's
row maxima and sums are integers: every comparison is for equality."""
import numpy as np
import pytest

from sbayes_amd import align, consensus
from sbayes_amd._handle import EngineError
from tests import _consensus_cases as cases
from tests import _consensus_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = consensus.ConsensusHandle()
    yield h
    h.close()


def fill(h, runs, capacity=None, pieces=None, n_runs=None, positions=None):
    """`runs` into a freshly shaped store: optionally a larger store, rows appended in pieces of the sizes given (in turn,
    repeated), more runs in the store than given and the given ones at chosen positions."""
    k, n = runs[0].shape[1:]
    positions = list(range(len(runs))) if positions is None else positions
    h.reset(len(runs) if n_runs is None else n_runs, k, n, capacity or max(max(r.shape[0] for r in runs), 1))
    for pos, run in zip(positions, runs):
        at, turn = 0, 0
        while at < run.shape[0]:
            size = pieces[turn % len(pieces)] if pieces else run.shape[0]
            h.append(pos, run[at:at + size])
            at, turn = at + size, turn + 1
        assert h.rows(pos) == run.shape[0]
    return positions


def check_counts(got, runs, what):
    want, _t = orc.similarity(runs)
    assert got.dtype == np.int32 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first at {bad[0]}: device {got[tuple(bad[0])]}, checker {want[tuple(bad[0])]}"


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("k", cases.KS)
def test_counts_equal_the_checker_over_tile_step_and_round_edges(handle, k, n):
    lengths = cases.edge_lengths(k)
    assert 1 in lengths and any(s * k in (64, 66, 72) for s in lengths) and any(s * k in (256, 258, 264) for s in lengths)
    for s in lengths:
        c = cases.overlapping(s, k, n, seed=5000 + 100 * n + 10 * k + s, density=0.35)
        fill(handle, [c])
        got = handle.similarity()
        check_counts(got, [c], f"K={k} N={n} S={s}")
        assert handle.last_kernel_ms() > 0.0 and handle.slot_samples[0] == s


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("piece", [1, 3, 5])
def test_pieces_that_start_and_end_inside_a_dword_of_the_image(handle, k, piece):
    assert (piece * k) % 8                                                  # a piece ends inside a dword (8 elements)
    c = cases.overlapping(97, k, 70, seed=5100 + 10 * k + piece)
    fill(handle, [c], pieces=[piece])
    check_counts(handle.similarity(), [c], f"K={k}, pieces of {piece}")
    fill(handle, [c], pieces=[piece, 7, 1, 2], capacity=400)                # mixed pieces, a store larger than its rows
    check_counts(handle.similarity(), [c], f"K={k}, mixed pieces from {piece}")
    counts, t = orc.similarity([c])
    assert np.array_equal(handle.scores(0), orc.scores(c, counts, t))       # (the bit rows took the same pieces)


def test_runs_of_different_lengths_a_selection_that_skips_one_and_a_reused_store(handle):
    runs = [cases.overlapping(s, 3, 65, seed=5200 + s) for s in (85, 1, 40, 22)]
    at = fill(handle, runs, n_runs=6, positions=[4, 0, 5, 2], capacity=90, pieces=[3, 5])
    check_counts(handle.similarity(), runs, "all runs")
    check_counts(handle.similarity(runs=[at[0], at[2], at[3]]), [runs[0], runs[2], runs[3]], "a selection that skips a run")
    check_counts(handle.similarity(runs=[at[1], 1, 3]), [runs[1]], "one sample and two empty runs")
    # a smaller store in the same handle: nothing of the rows before is left in the image
    small = [cases.overlapping(9, 3, 65, seed=5210)]
    fill(handle, small, n_runs=2, capacity=30)
    check_counts(handle.similarity(), small, "after a reset")


def test_one_launch_and_one_tile_pair_per_launch_give_the_same_bits(handle):
    c = cases.overlapping(33, 8, 257, seed=5300)                            # 9 tiles, 45 tile pairs
    fill(handle, [c])
    try:
        handle.set_launch_tiles(0)
        whole = handle.similarity()
        for tiles in (1, 7):
            handle.set_launch_tiles(tiles)
            assert np.array_equal(handle.similarity(slot=1), whole), tiles
        with pytest.raises(EngineError, match="tile_pairs=-1 out of range"):
            handle.set_launch_tiles(-1)
    finally:
        handle.set_launch_tiles(0)
    check_counts(whole, [c], "K=8 N=257")


def test_both_triangles_are_filled_and_the_diagonal_tiles_are_right(handle):
    # objects in ascending blocks: an asymmetric error (a tile written at its mirror's place, rows for columns) would show
    n = 100
    c = np.zeros((6, 4, n), dtype=np.uint8)
    for s in range(6):
        for k in range(4):
            c[s, k, 7 * k + s: 7 * k + s + 10 + 9 * k] = 1
    fill(handle, [c])
    handle.similarity(copy=False)                                           # slot 0 stays on the device ...
    got = handle.similarity(slot=1)
    want, _t = orc.similarity([c])
    assert np.array_equal(got, got.T) and np.array_equal(got, want)
    assert not np.array_equal(want[:32, 32:64], want[:32, 32:64].T)         # (an off-diagonal tile is not symmetric in itself)
    for t0 in range(0, n, 32):
        assert np.array_equal(got[t0:t0 + 32, t0:t0 + 32], want[t0:t0 + 32, t0:t0 + 32])
    assert np.array_equal(np.diag(got), c.sum(axis=(0, 1)))                 # (the areas overlap here: rows, not samples, are counted)
    row_max, row_sum = handle.compare()                                     # ... and is the same matrix
    assert not row_max.any() and not row_sum.any()


def test_scores_of_empty_clusters_all_ones_and_every_sample_of_three_runs(handle):
    runs = cases.three_runs()
    k, n = runs[0].shape[1:]
    extra = np.zeros((4, k, n), dtype=np.uint8)
    extra[1] = 1                                                            # every object in every area
    extra[2, 1] = runs[0][0, 1]                                             # one cluster, the others empty
    extra[3, :, ::2] = 1
    fill(handle, runs + [extra])
    pooled = handle.similarity(runs=[0, 1, 2])
    counts, t = orc.similarity(runs)
    assert np.array_equal(pooled, counts) and t == 121
    want = [orc.scores(r, counts, t) for r in runs]
    for r in range(3):
        got = handle.scores(r)
        assert got.dtype == np.int64 and np.array_equal(got, want[r]), f"run {r} against the pooled matrix"
        assert np.array_equal(got, orc.scores_gram(runs[r], runs))          # the checker's second form
    got = handle.scores(3)                                                  # a run outside the selection
    assert np.array_equal(got, orc.scores(extra, counts, t))
    assert got[0] == 0 and got[1] == k * (n * n * t - 2 * int(counts.sum()))
    other, t1 = orc.similarity([runs[1]])
    handle.similarity(runs=[1], slot=1, copy=False)
    for r in range(3):
        assert np.array_equal(handle.scores(r, slot=1), orc.scores(runs[r], other, t1)), f"run {r} against run 1's matrix"
        assert np.array_equal(handle.scores(r, slot=0), want[r])            # slot 0 is untouched
    est = consensus.point_estimate(runs)
    run, sample = orc.consensus(want)
    assert (est.run, est.sample, est.n_samples) == (run, sample, t)
    assert np.array_equal(est.clusters, runs[run][sample]) and est.clusters.dtype == np.uint8
    assert all(np.array_equal(a, b) for a, b in zip(est.scores, want))


def test_scores_where_a_workgroup_has_more_words_than_threads(handle):
    n = 32 * 256 + 40                                                       # 258 words for 256 threads
    c = cases.overlapping(3, 2, n, seed=5400, density=0.02)
    c[2, 0] = 0
    fill(handle, [c])
    handle.similarity(copy=False)
    assert np.array_equal(handle.scores(0), orc.scores_gram(c, [c]))         # (the form that needs no [N, N] matrix on the host)


def test_burn_in_and_the_planted_consensus():
    k, n = 3, 100
    c, _ = cases.planted(k, n, 48, flip=0.05, seed=4500, empty_every=0)
    truth, _ = cases.planted(k, n, 1, flip=0.0, seed=4501, empty_every=0)
    c[17] = truth[0]
    noise = cases.overlapping(8, k, n, seed=5500)                           # a burn-in that has nothing of the structure
    run = np.concatenate([noise, c])
    sim = consensus.similarity([run], burnin=8 / 56)
    counts, t = orc.similarity([c])
    assert sim.n_samples == t == 48 and np.array_equal(sim.counts, counts) and sim.counts.dtype == np.int32
    assert sim.probability.dtype == np.float64 and np.array_equal(sim.probability, counts / 48.0)
    est = consensus.point_estimate([run], burnin=8 / 56)
    assert (est.run, est.sample) == (0, 17) and np.array_equal(est.clusters, truth[0])


def test_comparison_of_runs_with_themselves_and_with_different_lengths(handle):
    runs = cases.three_runs()
    fill(handle, runs)
    mats = [orc.similarity([r]) for r in runs]
    handle.similarity([0], slot=0, copy=False)
    handle.similarity([0], slot=1, copy=False)
    row_max, row_sum = handle.compare()
    assert row_max.dtype == row_sum.dtype == np.int64 and not row_max.any() and not row_sum.any()
    handle.similarity([2], slot=1, copy=False)
    assert handle.slot_samples == [40, 48]
    row_max, row_sum = handle.compare()
    want_max, want_sum = orc.compare(*mats[0], *mats[2])
    assert np.array_equal(row_max, want_max) and np.array_equal(row_sum, want_sum) and row_max.any()
    assert handle.last_kernel_ms() > 0.0
    res = consensus.compare_runs(runs)
    want_abs, want_mean = orc.compare_runs(runs)
    assert res.max_abs.dtype == np.float64 and np.array_equal(res.max_abs, want_abs) and np.array_equal(res.mean_abs, want_mean)
    assert res.n_samples == (40, 33, 48) and not np.diag(res.max_abs).any() and res.max_abs[0, 1] > 0.0
    # one planted structure under three labellings: the runs agree, although their labels do not, better than a run
    # agrees with samples that have nothing of the structure
    unrelated = consensus.compare_runs([runs[0], cases.overlapping(40, 4, 100, seed=5600)])
    assert res.mean_abs.max() < unrelated.mean_abs[0, 1] and res.max_abs.max() < unrelated.max_abs[0, 1]


def test_the_limit_of_the_accumulator_two_runs_of_2_to_the_20_rows_all_ones():
    rows = np.ones((1 << 20, 8, 2), dtype=np.uint8)                         # 16 MiB of host rows per run
    h = consensus.ConsensusHandle()
    try:
        h.reset(3, 8, 2, 1 << 20)
        h.append(0, rows)
        h.append(1, rows[:1 << 19])
        h.append(1, rows[1 << 19:])
        got = h.similarity()
        assert h.slot_samples[0] == 1 << 21
        h.append(2, rows[:1])                                               # T K = 2^24 + K: refused by the library itself
        mask = np.ones(3, dtype=np.uint8)
        assert h._lib.sbe_consensus_similarity(h._h, mask.ctypes.data, 0, None) == 1
        assert "2097153 rows x 8 clusters = 16777224 elements, the limit is 16777216" in h._last_error()
        with pytest.raises(ValueError, match="16777224 elements"):
            h.similarity()
        assert got.tolist() == [[1 << 24, 1 << 24], [1 << 24, 1 << 24]]
        assert h.similarity(runs=[1]).tolist() == [[1 << 23, 1 << 23], [1 << 23, 1 << 23]]
    finally:
        h.close()


def test_state_errors_and_what_the_library_refuses_itself(handle):
    h = handle
    c = cases.overlapping(5, 3, 10, seed=5700)
    for args, text in [((1, 9, 10, 4), "n_clusters=9"), ((1, 8, 16385, 4), "n_objects=16385 out of range [1, 16384]"),
                       ((65, 2, 10, 4), "n_runs=65"), ((1, 2, 10, (1 << 20) + 1), "capacity_rows"),
                       ((1, 8, 16384, 1 << 20), "the limit is 17179869184")]:
        assert h._lib.sbe_consensus_reset(h._h, *args) == 1 and text in h._last_error(), text
    h.reset(3, 3, 10, 8)
    mask = np.ones(3, dtype=np.uint8)
    out = np.zeros((10, 10), dtype=np.int32)
    assert h._lib.sbe_consensus_similarity(h._h, mask.ctypes.data, 0, out.ctypes.data) == 3      # a selection without rows
    assert "hold no rows" in h._last_error()
    assert h._lib.sbe_consensus_similarity(h._h, mask.ctypes.data, 2, out.ctypes.data) == 1 and "slot=2" in h._last_error()
    assert h._lib.sbe_consensus_similarity(h._h, None, 0, out.ctypes.data) == 1 and "run_mask" in h._last_error()
    bad = c.copy()
    bad[3, 2, 7] = 2
    assert h._lib.sbe_consensus_append_rows(h._h, 0, bad.ctypes.data, 5) == 4 and "rows[3][2][7]=2 is neither 0 nor 1" in h._last_error()
    assert h.rows(0) == 0
    assert h._lib.sbe_consensus_append_rows(h._h, 0, np.zeros((9, 3, 10), dtype=np.uint8).ctypes.data, 9) == 1 and "store overflow" in h._last_error()
    assert h._lib.sbe_consensus_append_rows(h._h, 3, c.ctypes.data, 1) == 1 and "run 3 out of range" in h._last_error()
    assert h._lib.sbe_consensus_append_rows(h._h, 0, None, 1) == 1 and "null pointer" in h._last_error()
    h.append(0, c)
    h.append(1, c[:2])
    with pytest.raises(EngineError, match="slot 0 is empty") as err:                            # scoring against an empty slot
        h.scores(0)
    assert err.value.code == 3
    h.similarity([0], slot=0, copy=False)
    with pytest.raises(EngineError, match="slot 1 is empty"):                                   # comparing an empty slot
        h.compare()
    with pytest.raises(EngineError, match="hold no rows"):
        h._check(h._lib.sbe_consensus_similarity(h._h, np.array([0, 0, 1], dtype=np.uint8).ctypes.data, 1, None))
    h.similarity([1], slot=1, copy=False)
    h.compare()
    assert h.scores(0).shape == (5,) and h.scores(2).shape == (0,)
    h.append(2, c[:1])                                                                          # the store changes
    assert h.slot_samples == [0, 0]
    with pytest.raises(EngineError, match="slot 0 was computed before the store last changed") as err:
        h.scores(0)
    assert err.value.code == 3
    with pytest.raises(EngineError, match="computed before the store last changed"):
        h.compare()
    h.similarity([0], slot=0, copy=False)
    with pytest.raises(EngineError, match="slot 1 was computed before the store last changed"):
        h.compare()
    assert np.array_equal(h.scores(2), orc.scores(c[:1], *orc.similarity([c])))
    out64 = np.zeros(5, dtype=np.int64)
    assert h._lib.sbe_consensus_scores(h._h, 2, 0, out64.ctypes.data) == 1 and "slot=2" in h._last_error()
    assert h._lib.sbe_consensus_scores(h._h, 0, 3, out64.ctypes.data) == 1 and "run 3 out of range" in h._last_error()
    assert h._lib.sbe_consensus_scores(h._h, 0, 0, None) == 1 and "null pointer" in h._last_error()
    assert h._lib.sbe_consensus_compare(h._h, None, out64.ctypes.data) == 1 and "null pointer" in h._last_error()
    fresh = consensus.ConsensusHandle()
    try:
        with pytest.raises(EngineError, match="no shape yet"):
            fresh._check(fresh._lib.sbe_consensus_similarity(fresh._h, mask.ctypes.data, 0, None))
    finally:
        fresh.close()


def test_command_line_writes_the_consensus_and_the_similarity(tmp_path, capsys):
    runs = cases.relabelled_runs(3, 37, [30, 26], [[0, 1, 2], [2, 0, 1]], seed=5800)
    files = []
    for r, run in enumerate(runs):
        files.append(tmp_path / f"clusters_K3_{r}.txt")
        align.write_clusters(files[-1], run)
    out = tmp_path / "summary"
    assert consensus.main([str(f) for f in files] + ["--burnin", "0.1", "--out", str(out)]) == 0
    text = capsys.readouterr().out
    kept = [run[int(0.1 * len(run)):] for run in runs]
    counts, t = orc.similarity(kept)
    scores = [orc.scores(r, counts, t) for r in kept]
    run, sample = orc.consensus(scores)
    assert t == 27 + 24 and f"{t} samples after burn-in" in text
    assert f"consensus: sample {sample} (after burn-in) of clusters_K3_{run}.txt, score {int(scores[run][sample])}" in text
    lines = (out / "consensus_K3.txt").read_text().splitlines()
    assert len(lines) == 1
    assert np.array_equal(align.read_clusters(out / "consensus_K3.txt"), kept[run][sample][None])
    assert np.array_equal(consensus.read_similarity(out / "similarity_K3.txt"), counts / float(t))
    want_abs, want_mean = orc.compare_runs(kept)
    assert "%.6f" % want_abs[0, 1] in text and "%.6f" % want_mean[1, 0] in text
