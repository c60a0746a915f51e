"""sbayes_amd.partdist on the device against the checker (tests/_partdist_oracle.py).  Binder's distance, sumsq, the tables and
the binder sums are integers, and the variation of information is added up from the table the checker uses in the checker's
order: every comparison is for equality, except where a bound is named."""
import math

import numpy as np
import pytest

from sbayes_amd import _clusters, align, consensus, diag, partdist
from sbayes_amd._handle import EngineError
from tests import _consensus_oracle as consensus_orc
from tests import _partdist_cases as cases
from tests import _partdist_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = partdist.PartitionHandle()
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


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first at {bad[0]}: device {got[tuple(bad[0])]!r}, checker {want[tuple(bad[0])]!r}"


def check_whole_block(h, c, what):
    """block, sizes and tables of one run's whole store against the checker."""
    s, k, n = c.shape
    pos = np.arange(s)
    binder, vi, sumsq = orc.block(c, c, pos, pos)
    got = h.block(0)
    assert got.binder.dtype == np.int32 and got.vi.dtype == np.float64 and got.sumsq.dtype == np.int32
    same(got.binder, binder, f"{what} binder")
    same(got.sumsq, sumsq, f"{what} sumsq")
    same(got.vi, vi, f"{what} vi")
    assert not np.signbit(got.vi).any()
    same(h.sizes(0), orc.sizes(c), f"{what} sizes")
    pairs = np.array([(0, x, 0, y) for x in range(s) for y in range(s)], dtype=np.int64)
    tables = h.tables(pairs)
    want = np.einsum("xkn,yln->xykl", c.astype(np.int64), c.astype(np.int64))
    assert tables.dtype == np.int32
    same(tables.reshape(s, s, k, k), want, f"{what} tables")
    # the measures again on the host, from the vector pipe's tables: an independent check of the matrix pipe's counts
    sizes = h.sizes(0)
    again = orc.measures(tables.reshape(s, s, k, k), sizes, sizes, n, pos[:, None] > pos[None, :])
    same(got.binder, again[0], f"{what} binder from the tables")
    same(got.vi, again[1], f"{what} vi from the tables")
    same(got.sumsq, again[2], f"{what} sumsq from the tables")


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("k", cases.KS)
def test_whole_blocks_equal_the_checker_over_tile_and_round_edges(handle, k, n):
    lengths = cases.edge_lengths(k)
    pad = cases.padded(k)
    assert {s * pad for s in lengths} >= {32, 64} and min(lengths) * pad < 32 < 64 < max(lengths) * pad
    for s in lengths:
        c = cases.disjoint(s, k, n, seed=7000 + 100 * n + 10 * k + s, outside=0.3)
        fill(handle, [c])
        check_whole_block(handle, c, f"K={k} N={n} S={s}")
        assert handle.last_kernel_ms() > 0.0


def test_every_position_of_an_image_row_counts_exactly_once(handle):
    c = cases.position()                                                    # N = 321, K = 1: 322 samples, two rounds of objects
    n = 321
    fill(handle, [c], pieces=[100])
    got = handle.block(0)
    want = np.full((n + 1, n + 1), 2, dtype=np.int64)
    np.fill_diagonal(want, 0)
    want[:n, n] = want[n, :n] = n * n - 1
    same(got.binder, want, "binder of the singletons and the whole")
    binder, vi, sumsq = orc.block(c, c, np.arange(n + 1), np.arange(n + 1))
    assert np.array_equal(binder, want)
    same(got.vi, vi, "vi")
    same(got.sumsq, sumsq, "sumsq")


@pytest.mark.parametrize("k", [3, 5])
def test_pieces_of_any_size_and_a_store_larger_than_its_rows(handle, k):
    c = cases.disjoint(45, k, 70, seed=7100 + k)
    fill(handle, [c], pieces=[1, 7, 3], capacity=400)
    check_whole_block(handle, c, f"K={k}, mixed pieces")
    # a smaller store in the same handle: nothing of the rows before is left in the image
    small = cases.disjoint(9, k, 70, seed=7110 + k)
    fill(handle, [small], n_runs=2, capacity=30)
    check_whole_block(handle, small, f"K={k}, after a reset")


def test_sums_are_exact_for_binder_and_the_checkers_tree_for_vi(handle):
    runs = cases.three_runs() + [np.zeros((0, 4, 100), dtype=np.uint8)]     # 40, 33, 48 and an empty run
    fill(handle, runs, capacity=50, pieces=[16, 5])
    want_b, want_v = orc.sums(runs)
    got_b, got_v = handle.sums()
    assert got_b.dtype == np.int64 and got_v.dtype == np.float64 and got_b.shape == (121, 4)
    same(got_b, want_b, "binder sums of all runs")
    same(got_v, want_v, "vi sums of all runs")
    assert handle.last_kernel_ms() > 0.0 and not got_b[:, 3].any() and not got_v[:, 3].any()
    # within the derived bound of the exact sum of the same terms
    pos = orc.positions(runs)
    for a in range(3):
        for b in range(3):
            _, vi, _ = orc.block(runs[a], runs[b], pos[a], pos[b])
            exact = np.array([math.fsum(row) for row in vi])
            assert (np.abs(got_v[pos[a], b] - exact) <= orc.tree_bound(vi)).all()
    # a selection that skips a run: the samples and the columns of the selected runs only
    sel_b, sel_v = handle.sums(runs=[2, 0])
    want_b, want_v = orc.sums(runs, [0, 2])
    same(sel_b, want_b, "binder sums of runs 0 and 2")
    same(sel_v, want_v, "vi sums of runs 0 and 2")
    assert sel_b.shape == (88, 2)


def test_the_binder_sums_are_the_consensus_scores_plus_the_sum_of_the_counts_on_the_device(handle):
    runs = cases.three_runs()
    fill(handle, runs)
    binder_sum, _ = handle.sums()
    ch = consensus.ConsensusHandle.filled(None, _clusters.store_shape(runs, 4, 100), runs)
    try:
        counts = ch.similarity()
        scores = np.concatenate([ch.scores(r) for r in range(3)])
    finally:
        ch.close()
    assert np.array_equal(counts, consensus_orc.similarity(runs)[0])
    same(binder_sum.sum(axis=1), scores + int(counts.astype(np.int64).sum()), "sum_t binder(s,t) = score[s] + sum C")
    est, med = consensus.point_estimate(runs), partdist.medoid(runs, loss="binder")
    assert (med.run, med.sample) == (est.run, est.sample) and np.array_equal(med.clusters, est.clusters) and med.n_samples == 121
    assert np.array_equal(np.concatenate(med.expected_loss), binder_sum.sum(axis=1) / 121.0)


def test_recorded_reference_clusters_are_at_distance_zero_of_their_realignment(handle):
    for tag, (logged, realigned) in cases.golden_realign().items():
        s, k, n = logged.shape
        fill(handle, [logged, realigned])
        got = handle.block(0, col_run=1)
        a = orc.sizes(logged)
        own = (a * a).sum(axis=1) + (n - a.sum(axis=1)) ** 2
        bound = orc.vi_bound(k, n, orc.vi_magnitude(orc.tables(logged, realigned), a, orc.sizes(realigned), n))
        assert not np.diag(got.binder).any(), tag
        assert np.array_equal(np.diag(got.sumsq), own), tag
        assert (np.diag(got.vi) >= 0.0).all() and (np.diag(got.vi) <= np.diag(bound)).all(), tag
        binder, vi, sumsq = orc.block(logged, realigned, np.arange(s), s + np.arange(s))
        same(got.binder, binder, f"{tag} binder")
        same(got.vi, vi, f"{tag} vi")
        same(got.sumsq, sumsq, f"{tag} sumsq")


def test_state_errors_and_what_the_library_refuses_itself(handle):
    h = handle
    lib = h._lib
    c = cases.disjoint(5, 3, 10, seed=7200)
    table = partdist.xlogx(10)
    fresh = partdist.PartitionHandle()
    try:
        out = np.full((1, 1), -7, dtype=np.int32)
        mask = np.ones(3, dtype=np.uint8)
        assert lib.sbe_partdist_block(fresh._h, 0, 0, 1, 0, 0, 1, out.ctypes.data, None, None) == 3 and "no shape yet" in fresh._last_error()
        assert lib.sbe_partdist_sums(fresh._h, mask.ctypes.data, out.ctypes.data, None) == 3 and "no shape yet" in fresh._last_error()
        assert lib.sbe_partdist_append_rows(fresh._h, 0, c.ctypes.data, 1) == 3 and "no shape yet" in fresh._last_error()
        assert out[0, 0] == -7
    finally:
        fresh.close()
    for args, text in [((1, 9, 10, 4), "n_clusters=9"), ((1, 8, 16385, 4), "n_objects=16385 out of range [1, 16384]"),
                       ((65, 2, 10, 4), "n_runs=65"), ((1, 2, 10, (1 << 20) + 1), "capacity_rows"),
                       ((1, 8, 16384, 1 << 20), "the limit is 17179869184")]:
        assert lib.sbe_partdist_reset(h._h, *args, table.ctypes.data) == 1 and text in h._last_error(), text
    assert lib.sbe_partdist_reset(h._h, 1, 3, 10, 4, None) == 1 and "xlogx" in h._last_error()
    h.reset(3, 3, 10, 8)
    mask = np.ones(3, dtype=np.uint8)
    sums = np.full((5, 3), -7, dtype=np.int64)
    assert lib.sbe_partdist_sums(h._h, mask.ctypes.data, sums.ctypes.data, None) == 3 and "hold no rows" in h._last_error()      # an empty selection
    assert lib.sbe_partdist_sums(h._h, None, sums.ctypes.data, None) == 1 and "run_mask" in h._last_error()
    h.append(0, c)
    h.append(1, c[:2])
    before = h.block(0, col_run=1)
    # data the library refuses: the store is unchanged
    bad = c.copy()
    bad[3, 2, 7] = 2
    assert lib.sbe_partdist_append_rows(h._h, 1, bad.ctypes.data, 5) == 4 and "rows[3][2][7]=2 is neither 0 nor 1" in h._last_error()
    overlap = c.copy()
    overlap[4, :, 6] = 0
    overlap[4, 0, 6] = overlap[4, 2, 6] = 1
    assert lib.sbe_partdist_append_rows(h._h, 1, overlap.ctypes.data, 5) == 4
    assert "rows[4]: object 6 is in 2 areas of the sample" in h._last_error()
    assert h.rows(0) == 5 and h.rows(1) == 2 and h.rows(2) == 0
    after = h.block(0, col_run=1)
    assert after.binder.tobytes() == before.binder.tobytes() and after.vi.tobytes() == before.vi.tobytes() and after.sumsq.tobytes() == before.sumsq.tobytes()
    assert lib.sbe_partdist_append_rows(h._h, 0, np.zeros((9, 3, 10), dtype=np.uint8).ctypes.data, 9) == 1 and "store overflow" in h._last_error()
    assert lib.sbe_partdist_append_rows(h._h, 3, c.ctypes.data, 1) == 1 and "run 3 out of range" in h._last_error()
    assert lib.sbe_partdist_append_rows(h._h, 0, None, 1) == 1 and "null pointer" in h._last_error()
    # arguments the library refuses: the outputs are untouched
    out = np.full((5, 5), -7, dtype=np.int32)
    for args, text in [((0, 0, 6, 0, 0, 5), "rows [0, 0 + 6) are not within the 5 rows of run 0"), ((0, 0, 0, 0, 0, 5), "rows [0, 0 + 0)"),
                       ((0, -1, 2, 0, 0, 5), "rows [-1"), ((0, 0, 5, 1, 1, 2), "cols [1, 1 + 2) are not within the 2 rows of run 1"),
                       ((0, 0, 5, 2, 0, 1), "cols [0, 0 + 1) are not within the 0 rows of run 2"), ((3, 0, 1, 0, 0, 1), "row_run 3 out of range"),
                       ((0, 0, 1, -1, 0, 1), "col_run -1 out of range")]:
        assert lib.sbe_partdist_block(h._h, *args, out.ctypes.data, None, None) == 1 and text in h._last_error(), text
    assert lib.sbe_partdist_block(h._h, 0, 0, 5, 0, 0, 5, None, None, None) == 1 and "at least one is needed" in h._last_error()
    assert lib.sbe_partdist_sums(h._h, mask.ctypes.data, None, None) == 1 and "at least one is needed" in h._last_error()
    pairs = np.array([[0, 0, 1, 2]], dtype=np.int64)
    assert lib.sbe_partdist_tables(h._h, pairs.ctypes.data, 1, out.ctypes.data) == 1 and "pairs[0]: (run 1, row 2) is not a stored sample" in h._last_error()
    assert lib.sbe_partdist_tables(h._h, pairs.ctypes.data, 0, out.ctypes.data) == 1 and "n_pairs=0" in h._last_error()
    assert lib.sbe_partdist_tables(h._h, None, 1, out.ctypes.data) == 1 and "null pointer" in h._last_error()
    assert lib.sbe_partdist_sizes(h._h, 3, out.ctypes.data) == 1 and "run 3 out of range" in h._last_error()
    assert lib.sbe_partdist_sizes(h._h, 0, None) == 1 and "null pointer" in h._last_error()
    assert (out == -7).all() and (sums == -7).all()
    with pytest.raises(EngineError, match="hold no rows") as err:
        h._check(lib.sbe_partdist_sums(h._h, np.array([0, 0, 1], dtype=np.uint8).ctypes.data, sums.ctypes.data, None))
    assert err.value.code == 3
    with pytest.raises(EngineError, match="tile_pairs=-1 out of range"):
        h.set_launch_tiles(-1)
    assert h.sizes(2).shape == (0, 3)


def test_the_sums_refuse_a_selection_beyond_their_limit():
    h = partdist.PartitionHandle()
    try:
        h.reset(2, 1, 2, 1 << 16)
        rows = np.zeros((1 << 16, 1, 2), dtype=np.uint8)
        h.append(0, rows)
        h.append(1, rows[:1])
        mask = np.ones(2, dtype=np.uint8)
        out = np.full(4, -7, dtype=np.int64)
        assert h._lib.sbe_partdist_sums(h._h, mask.ctypes.data, out.ctypes.data, None) == 1
        assert "the selection holds 65537 rows, the limit for the sums is 65536" in h._last_error() and (out == -7).all()
        assert h._lib.sbe_partdist_block(h._h, 0, 0, 1 << 16, 0, 0, 1 << 16, out.ctypes.data, None, None) == 1
        assert "a block of 65536 x 65536 = 4294967296 entries, the limit is 268435456" in h._last_error() and (out == -7).all()
    finally:
        h.close()


def test_the_python_layer_on_three_runs():
    runs = cases.three_runs()
    lengths = [40, 33, 48]
    pos = orc.positions(runs)
    everything = np.concatenate(runs)
    binder, vi, sumsq = orc.block(everything, everything, np.arange(121), np.arange(121))
    d = partdist.distances(runs)
    assert d.offsets == (0, 40, 73, 121) and d.kernel_ms > 0.0
    same(d.binder, binder, "distances binder")
    same(d.vi, vi, "distances vi")
    assert np.array_equal(d.vi, d.vi.T) and np.array_equal(d.binder, d.binder.T) and not np.diag(d.vi).any()
    sizes = orc.sizes(everything)
    same(d.sizes, sizes, "distances sizes")
    same(d.ari, partdist.adjusted_rand(sumsq, sizes, sizes, 100), "distances ari")
    assert np.array_equal(np.diag(d.ari), np.ones(121)) and d.ari.max() <= 1.0
    x, y = 5, 77
    e, _, _ = orc.extended(orc.tables(everything[x:x + 1], everything[y:y + 1])[0, 0], sizes[x], sizes[y], 100)
    assert abs(d.ari[x, y] - orc.adjusted_rand(e)) <= 4 * 2.0 ** -53 * abs(orc.adjusted_rand(e))
    # burn-in drops the first samples of every run
    burnt = partdist.distances(runs, burnin=0.25)
    keep = np.concatenate([p[int(0.25 * len(p)):] for p in pos])
    same(burnt.vi, vi[np.ix_(keep, keep)], "distances after burn-in")
    # run against run: one planted structure under three labellings, so between-run is about within-run, and both are far
    # below the distance to samples that have nothing of the structure
    rd = partdist.run_distances(runs)
    want_b, want_v = orc.sums(runs)
    for a in range(3):
        for b in range(3):
            pairs = lengths[a] * (lengths[a] - 1) if a == b else lengths[a] * lengths[b]
            assert rd.binder[a, b] == sum(int(v) for v in want_b[pos[a], b]) / pairs
            assert rd.vi[a, b] == math.fsum(want_v[pos[a], b]) / pairs
    assert rd.n_samples == (40, 33, 48)
    other = partdist.run_distances([runs[0], cases.disjoint(40, 4, 100, seed=7300)])
    assert rd.vi.max() < other.vi[0, 1] and rd.binder.max() < other.binder[0, 1]
    # the medoid under VI and the ball around it
    med = partdist.medoid(runs, loss="vi")
    total = np.zeros(121)
    for col in range(3):
        total = total + want_v[:, col]
    at = int(np.argmin(total))
    assert pos[med.run][med.sample] == at and np.array_equal(med.clusters, everything[at])
    assert np.array_equal(np.concatenate(med.expected_loss), total / 121.0)
    for loss, matrix in (("vi", vi), ("binder", binder)):
        ball = partdist.credible_ball(runs, mass=0.95, loss=loss)
        center = pos[ball.run][ball.sample]
        dist = np.concatenate(ball.distances)
        same(dist, matrix[:, center].astype(np.float64), f"distances to the {loss} medoid")
        members = np.concatenate(ball.members)
        assert members.sum() >= 0.95 * 121 and np.array_equal(members, dist <= ball.radius)
        below = dist[dist < ball.radius].max()                              # one distance step below the radius
        assert (dist <= below).sum() < 0.95 * 121
        assert np.array_equal(ball.estimate, everything[center])
    # a given estimate: it is stored as a run of its own behind the others, so it is the later sample of every pair
    truth = everything[at]
    ball = partdist.credible_ball(runs, estimate=truth, mass=0.5)
    _, to_truth, _ = orc.block(everything, truth[None], np.arange(121), np.array([121]))
    same(np.concatenate(ball.distances), to_truth[:, 0], "distances to a given estimate")
    assert (ball.run, ball.sample) == (-1, -1) and np.concatenate(ball.members).sum() >= 61


def test_command_line_writes_the_medoid_and_the_traces(tmp_path, capsys):
    runs = cases.three_runs()
    files = []
    for r, run in enumerate(runs):
        files.append(tmp_path / f"clusters_K4_run{r}.txt")
        align.write_clusters(files[-1], run)
    out = tmp_path / "distances"
    assert partdist.main([str(f) for f in files] + ["--burnin", "0.1", "--loss", "vi", "--mass", "0.9", "--out", str(out)]) == 0
    text = capsys.readouterr().out
    kept = [run[int(0.1 * len(run)):] for run in runs]
    lengths = [len(r) for r in kept]
    pos = orc.positions(kept)
    everything = np.concatenate(kept)
    total_n = sum(lengths)
    _, vi, _ = orc.block(everything, everything, np.arange(total_n), np.arange(total_n))
    _, want_v = orc.sums(kept)
    total = np.zeros(total_n)
    for col in range(3):
        total = total + want_v[:, col]
    at = int(np.argmin(total))
    run = next(r for r in range(3) if at in pos[r])
    sample = at - pos[run][0]
    assert f"{total_n} samples after burn-in" in text and f"medoid (vi): sample {sample} (after burn-in) of clusters_K4_run{run}.txt" in text
    assert np.array_equal(align.read_clusters(out / "medoid_K4.txt"), everything[at][None])
    for r in range(3):
        names, rows = diag.read_stats(out / f"partition_trace_K4_run{r}.txt")
        assert names == ["vi_to_estimate"] and np.array_equal(rows[:, 0], vi[pos[r], at])
    radius = partdist.ball_radius([vi[:, at]], 0.9)
    assert f"radius {radius!r} holds {int((vi[:, at] <= radius).sum())} of {total_n} samples" in text
    within = math.fsum(want_v[pos[0], 0]) / (lengths[0] * (lengths[0] - 1))
    assert "%.6f" % within in text
