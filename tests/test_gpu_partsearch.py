"""The partition search on the device (include/sbe_partsearch.h, sbayes_amd/partsearch.py) against its checker
(tests/_partsearch_oracle.py): every output of every start equals the checker's, bit for bit."""
import numpy as np
import pytest

from sbayes_amd import partdist, partsearch
from sbayes_amd._handle import EngineError, _ptr
from tests import _partdist_cases as partdist_cases
from tests import _partsearch_cases as cases
from tests import _partsearch_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = partsearch.SearchHandle()
    yield h
    h.close()


def fill(h, y, k, pieces=None, capacity=None):
    """The label rows y [T, N] as 0/1 samples into a freshly shaped store, appended in pieces of the sizes given (in turn)."""
    rows = orc.rows_of(y, k)
    h.reset(k, y.shape[1], capacity or y.shape[0])
    at, turn = 0, 0
    while at < y.shape[0]:
        size = pieces[turn % len(pieces)] if pieces else y.shape[0]
        h.append(rows[at:at + size])
        at, turn = at + size, turn + 1
    assert h.rows() == y.shape[0]


def check_search(h, y, k, loss, init, order, max_sweeps, what):
    """search() of the filled handle against the checker, start by start; returns (device, checker)."""
    got = h.search(loss, init, order, max_sweeps, trace=True)
    want = cases.oracle_starts(y, k, loss, init, order, max_sweeps)
    assert got.labels.dtype == np.uint8 and got.sweeps.dtype == np.int32 and got.moves.dtype == np.int64 and got.vi_sum.dtype == np.float64
    for s, w in enumerate(want):
        at = f"{what} {loss} start {s}"
        assert np.array_equal(got.labels[s], w.labels), at
        assert (int(got.sweeps[s]), int(got.moves[s]), int(got.converged[s])) == (w.sweeps, w.moves, w.converged), at
        assert int(got.binder_sum[s]) == w.binder_sum and got.vi_sum[s] == w.vi_sum and not np.signbit(got.vi_sum[s]), at
        assert np.array_equal(got.trace[s], w.trace, equal_nan=True), at
    return got, want


@pytest.mark.parametrize("loss", cases.LOSSES)
@pytest.mark.parametrize("n,k,t,starts", cases.GRID)
def test_every_output_equals_the_checker_at_the_strides_of_the_tree(handle, n, k, t, starts, loss):
    y, _ = cases.noisy(n * 1000 + t, n, k, t)
    fill(handle, y, k)
    init, order = cases.starts_of(y, k, starts, seed=n + t, loss=loss)
    got, want = check_search(handle, y, k, loss, init, order, 32, f"N={n} K={k} T={t}")
    assert got.trace.shape == (starts, 32)
    # evaluate is what the search ends with
    ev = handle.evaluate(got.labels)
    assert np.array_equal(ev.vi_sum, got.vi_sum) and np.array_equal(ev.binder_sum, got.binder_sum)
    vi, binder, vi_sum, binder_sum = orc.evaluate(got.labels, y, k)
    assert ev.vi.dtype == np.float64 and ev.binder.dtype == np.int32
    assert np.array_equal(ev.vi, vi) and np.array_equal(ev.binder, binder) and np.array_equal(ev.vi_sum, vi_sum) and np.array_equal(ev.binder_sum, binder_sum)


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_one_sweep_leaves_the_search_unconverged_and_orders_matter_as_the_checker_says(handle, loss):
    n, k, t = 33, 5, 65
    y, _ = cases.noisy(9, n, k, t)
    fill(handle, y, k)
    init = cases.random_starts(2, n, k, 1)[0].repeat(3, axis=0)
    order = np.stack([np.arange(n), np.arange(n)[::-1], np.random.default_rng(3).permutation(n)]).astype(np.int32)
    got, _ = check_search(handle, y, k, loss, init, order, 1, "one sweep")
    assert not got.converged.any() and (got.sweeps == 1).all() and (got.moves > 0).all()
    check_search(handle, y, k, loss, init, order, 64, "identity, reversed and shuffled order")


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_inits_with_empty_blocks_and_samples_without_label_0_or_k(handle, loss):
    n, k, t = 31, 5, 64
    for labels, what in [(None, "labels 0 and K present"), ([1, 2, 3, 4], "labels 0 and K absent"), ([0, 5], "only labels 0 and K")]:
        y, truth = cases.noisy(21, n, k, t, labels=labels)
        fill(handle, y, k)
        init = np.stack([np.zeros(n, dtype=np.uint8), np.full(n, k, dtype=np.uint8), np.where(np.arange(n) % 2, 1, 4).astype(np.uint8), truth])
        order = cases.random_starts(6, n, k, 4)[1]
        check_search(handle, y, k, loss, init, order, 64, what)


def test_equal_samples_and_a_start_one_move_away_reach_them_at_exactly_zero(handle):
    n, k, t = 33, 5, 65
    truth = cases.noisy(4, n, k, 1)[1]
    y = np.repeat(truth[None], t, axis=0)
    fill(handle, y, k)
    init = np.stack([truth, truth, np.zeros(n, dtype=np.uint8)])
    init[1, 7] = (init[1, 7] + 1) % (k + 1)
    order = np.stack([np.arange(n)] * 3).astype(np.int32)
    for loss in cases.LOSSES:
        got, _ = check_search(handle, y, k, loss, init, order, 16, "all samples equal")
        assert np.array_equal(got.labels[1], truth) and got.vi_sum[1] == 0.0 and got.binder_sum[1] == 0
        assert (int(got.sweeps[1]), int(got.moves[1]), int(got.converged[1])) == (2, 1, 1) and (int(got.sweeps[0]), int(got.moves[0])) == (1, 0)


def test_two_contradictory_samples_tie_exactly_under_binder(handle):
    y, k, init, order = cases.contradictory()
    fill(handle, y, k)
    _, want = check_search(handle, y, k, "binder", init, order, 8, "contradictory samples")
    ties = np.sum([w.ties for w in want], axis=0)
    assert ties[0] > 0 and ties[1] > 0
    check_search(handle, y, k, "vi", init, order, 8, "contradictory samples")


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_no_bit_depends_on_the_pieces_of_the_rows_or_the_split_of_the_starts(handle, loss):
    n, k, t, starts = 33, 5, 65, 5
    y, _ = cases.noisy(31, n, k, t)
    init, order = cases.starts_of(y, k, starts, seed=1, loss=loss)
    fill(handle, y, k)
    whole, _ = check_search(handle, y, k, loss, init, order, 32, "whole")
    for pieces, capacity in [([1], t), ([7], t + 9), ([1, 7, 20], 300)]:
        fill(handle, y, k, pieces, capacity)
        again = handle.search(loss, init, order, 32, trace=True)
        for name in ("labels", "sweeps", "moves", "converged", "binder_sum", "vi_sum"):
            assert np.array_equal(getattr(again, name), getattr(whole, name)), (pieces, name)
        assert np.array_equal(again.trace, whole.trace, equal_nan=True)
    for calls in (2, starts):
        edges = np.linspace(0, starts, calls + 1).astype(int)
        parts = [handle.search(loss, init[a:b], order[a:b], 32, trace=True) for a, b in zip(edges[:-1], edges[1:])]
        for name in ("labels", "sweeps", "moves", "converged", "binder_sum", "vi_sum"):
            assert np.array_equal(np.concatenate([getattr(p, name) for p in parts]), getattr(whole, name)), (calls, name)
        assert np.array_equal(np.concatenate([p.trace for p in parts]), whole.trace, equal_nan=True)


def test_evaluate_equals_the_partition_distances_block(handle):
    n, k, t = 257, 8, 65
    y, _ = cases.noisy(5, n, k, t)
    fill(handle, y, k)
    cands = cases.random_starts(8, n, k, 3)[0]
    cands[2][cands[2] >= 4] = 0                                # empty blocks
    ev = handle.evaluate(cands)
    ph = partdist.PartitionHandle()
    try:
        ph.reset(2, k, n, t)
        ph.append(0, orc.rows_of(cands, k))                   # the estimates as run 0, the samples as run 1
        ph.append(1, orc.rows_of(y, k))
        block = ph.block(0, col_run=1, sumsq=False)
    finally:
        ph.close()
    assert np.array_equal(ev.vi, block.vi) and np.array_equal(ev.binder, block.binder)


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_recorded_reference_clusters_as_samples(handle, loss):
    for tag, (logged, _) in partdist_cases.golden_realign().items():
        y = orc.labels_of(logged)[:48]
        k = logged.shape[1]
        fill(handle, y, k)
        init, order = cases.starts_of(y, k, 3, seed=2, loss=loss)
        check_search(handle, y, k, loss, init, order, 8, tag)


def test_the_largest_objects_and_clusters_with_one_sweep(handle):
    n, k, t = 16384, 8, 3
    y, _ = cases.noisy(6, n, k, t, flip=0.1)
    fill(handle, y, k)
    init = y[:1].copy()
    init[0, ::5] = 0
    order = np.arange(n, dtype=np.int32)[None, ::-1]
    got, _ = check_search(handle, y, k, "vi", init, order, 1, "N = 16384")
    assert got.moves[0] > 0
    check_search(handle, y, k, "binder", init, order, 1, "N = 16384")


def test_the_python_layer_on_two_runs_concatenated():
    n, k = 40, 3
    y, truth = cases.noisy(13, n, k, 90, flip=0.3)
    runs = [orc.rows_of(y[:50], k), orc.rows_of(y[50:], k)]
    for loss in cases.LOSSES:
        res = partsearch.search(runs, loss=loss, starts=6, seed=4, burnin=0.1)
        kept = np.concatenate([y[5:50], y[54:]])
        init, order = cases.starts_of(kept, k, 6, 4, loss)
        want = cases.oracle_starts(kept, k, loss, init, order, 64)
        sums = [w.vi_sum if loss == "vi" else w.binder_sum for w in want]
        assert list(res.starts["loss_sum"]) == sums and list(res.starts["sweeps"]) == [w.sweeps for w in want]
        assert res.starts["kind"] == ["medoid", "sample", "sample", "sample", "zero", "random"] and res.n_samples == 81
        med = partdist.medoid(runs, loss=loss, burnin=0.1)
        # (partdist adds a sample's VI distances in a tree of its own: the two means agree to rounding, Binder's exactly)
        assert abs(res.medoid_loss - med.expected_loss[med.run][med.sample]) <= (0 if loss == "binder" else 2.0 ** -40)
        assert res.expected_loss <= res.medoid_loss and res.clusters.shape == (k, n) and res.clusters.sum(axis=0).max() <= 1
        ev = partsearch.evaluate(runs, np.stack([res.clusters, med.clusters]), burnin=0.1)
        mean = (ev.vi_sum if loss == "vi" else ev.binder_sum) / 81.0
        assert mean[0] == res.expected_loss and mean[1] == res.medoid_loss
        ball = partsearch.credible_ball(runs, res.clusters, mass=0.9, loss=loss, burnin=0.1)
        d = ev.distances(loss)[0]
        assert np.array_equal(np.concatenate(ball.distances), d) and ball.radius == np.sort(d)[int(np.ceil(0.9 * 81)) - 1]
        assert [len(v) for v in ball.distances] == [45, 36]


def test_command_line_writes_the_estimate(tmp_path, capsys):
    from sbayes_amd import align
    y, _ = cases.noisy(14, 30, 3, 40)
    align.write_clusters(tmp_path / "clusters_K3_0.txt", orc.rows_of(y[:25], 3))
    align.write_clusters(tmp_path / "clusters_K3_1.txt", orc.rows_of(y[25:], 3))
    assert partsearch.main([str(tmp_path / "clusters_K3_0.txt"), str(tmp_path / "clusters_K3_1.txt"), "--starts", "4", "--out", str(tmp_path / "out")]) == 0
    res = partsearch.search([orc.rows_of(y[:25], 3), orc.rows_of(y[25:], 3)], starts=4)
    assert np.array_equal(align.read_clusters(tmp_path / "out" / "estimate_K3.txt"), res.clusters[None])
    text = capsys.readouterr().out
    assert f"medoid {res.medoid_loss!r}, search {res.expected_loss!r}" in text and "credible ball (vi, mass 0.95): radius" in text


def test_what_the_library_refuses_itself_leaves_the_store_unchanged(handle):
    n, k, t = 9, 2, 7
    y, _ = cases.noisy(1, n, k, t)
    fill(handle, y, k, capacity=t + 2)
    init, order = cases.random_starts(1, n, k, 2)
    before = handle.search("vi", init, order, 8)
    lib, h = handle._lib, handle._h
    labels, sweeps, moves = np.empty((2, n), dtype=np.uint8), np.empty(2, dtype=np.int32), np.empty(2, dtype=np.int64)
    converged, bsum, vsum = np.empty(2, dtype=np.uint8), np.empty(2, dtype=np.int64), np.empty(2, dtype=np.float64)

    def raw(loss, n_starts, a_init, a_order, max_sweeps):
        return lib.sbe_partsearch_search(h, loss, n_starts, _ptr(a_init), _ptr(a_order), max_sweeps, _ptr(labels), _ptr(sweeps), _ptr(moves), _ptr(converged),
                                         _ptr(bsum), _ptr(vsum), None)
    twice = order.copy()
    twice[1, 4] = twice[1, 0]
    assert raw(0, 2, init, twice, 8) == 4 and f"order[1][4]={int(twice[1, 4])} comes a second time" in handle._last_error()
    beyond = order.copy()
    beyond[0, 2] = n
    assert raw(0, 2, init, beyond, 8) == 4 and f"order[0][2]={n} is not an object in [0, {n})" in handle._last_error()
    high = init.copy()
    high[1, 3] = k + 1
    assert raw(1, 2, high, order, 8) == 4 and f"init[1][3]={k + 1} is not a label in [0, {k}]" in handle._last_error()
    assert raw(2, 2, init, order, 8) == 1 and "loss=2" in handle._last_error()
    assert raw(0, 2, init, order, 0) == 1 and raw(0, 2, init, order, 1025) == 1 and "max_sweeps=1025 out of range [1, 1024]" in handle._last_error()
    assert raw(0, 0, init, order, 8) == 1 and "n_starts=0" in handle._last_error()
    overlap = orc.rows_of(y[:2], k)
    overlap[1, :, 5] = 1
    assert lib.sbe_partsearch_append_rows(h, _ptr(overlap), 2) == 4 and "rows[1]: object 5 is in 2 areas" in handle._last_error()
    overlap[1, :, 5] = 0
    overlap[0, 1, 2] = 3
    assert lib.sbe_partsearch_append_rows(h, _ptr(overlap), 2) == 4 and "rows[0][1][2]=3 is neither 0 nor 1" in handle._last_error()
    three = orc.rows_of(y[:3], k)
    assert lib.sbe_partsearch_append_rows(h, _ptr(three), 3) == 1 and "store overflow" in handle._last_error()
    assert lib.sbe_partsearch_evaluate(h, 1, _ptr(high), None, None, None, None) == 1 and "at least one is needed" in handle._last_error()
    assert lib.sbe_partsearch_evaluate(h, 2, _ptr(high), None, None, _ptr(vsum), None) == 4 and "labels[1][3]=3" in handle._last_error()
    assert handle.rows() == t
    after = handle.search("vi", init, order, 8)
    assert np.array_equal(after.labels, before.labels) and np.array_equal(after.vi_sum, before.vi_sum)
    # state: no shape, no rows
    fresh = partsearch.SearchHandle()
    try:
        assert fresh._lib.sbe_partsearch_append_rows(fresh._h, _ptr(three), 3) == 3 and "no shape yet" in fresh._last_error()
        assert fresh._lib.sbe_partsearch_evaluate(fresh._h, 1, _ptr(init), None, None, _ptr(vsum), None) == 3
        fresh.reset(k, n, 4)
        assert fresh.rows() == 0
        assert fresh._lib.sbe_partsearch_evaluate(fresh._h, 1, _ptr(init), None, None, _ptr(vsum), None) == 3 and "holds no rows" in fresh._last_error()
        with pytest.raises(ValueError, match="holds no samples"):
            fresh.search("vi", init, order)
        with pytest.raises(EngineError, match="n_objects=16385"):
            fresh._check(fresh._lib.sbe_partsearch_reset(fresh._h, 1, 16385, 1, _ptr(vsum)))
    finally:
        fresh.close()
