"""sbayes_amd.partdist on the device over its ranges (tests/test_gpu_partdist.py has the whole blocks): blocks whose rows and
columns start and end inside a tile and come from different runs, the launch chunking, and the largest N.  Every comparison
is for equality of the bytes."""
import numpy as np
import pytest

from sbayes_amd import partdist
from tests import _partdist_cases as cases
from tests import _partdist_oracle as orc
from tests.test_gpu_partdist import fill, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = partdist.PartitionHandle()
    yield h
    h.close()


def same_bytes(a, b, what):
    for name in ("binder", "vi", "sumsq"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {name}"


@pytest.mark.parametrize("k", [1, 3, 8])
def test_ranges_inside_tiles_across_runs_one_by_many_and_many_by_one(handle, k):
    per_tile = 32 // cases.padded(k)
    lengths = [2 * per_tile + 3, per_tile + 1, 3 * per_tile + 2]
    n = 70
    runs = [cases.disjoint(s, k, n, seed=7500 + 10 * k + r, outside=0.25) for r, s in enumerate(lengths)]
    at = fill(handle, runs, n_runs=5, positions=[3, 0, 4], capacity=4 * per_tile, pieces=[5, 2])
    stored = dict(zip(at, runs))
    pos = {run: 1000 * run + np.arange(len(c)) for run, c in stored.items()}              # ordered as (run, sample) is
    whole = {(a, b): handle.block(a, col_run=b) for a in at for b in at}
    for (a, b), got in whole.items():
        binder, vi, sumsq = orc.block(stored[a], stored[b], pos[a], pos[b])
        same(got.binder, binder, f"runs {a} x {b} binder")
        same(got.vi, vi, f"runs {a} x {b} vi")
        same(got.sumsq, sumsq, f"runs {a} x {b} sumsq")
        # the part below the diagonal equals the transpose: vi takes the earlier sample as x from whichever side
        back = whole[(b, a)]
        assert np.array_equal(got.binder, back.binder.T) and np.array_equal(got.sumsq, back.sumsq.T)
        assert got.vi.tobytes() == np.ascontiguousarray(back.vi.T).tobytes()
    windows = [(1, per_tile), (per_tile - 1, 3), (per_tile, per_tile), (0, 1), (per_tile + 1, 1)]     # (first, count): inside, across and at a tile edge
    for a, b in [(3, 3), (3, 4), (4, 0), (0, 3)]:
        full = whole[(a, b)]
        for r0, nr in windows:
            for c0, nc in windows:
                if r0 + nr > len(stored[a]) or c0 + nc > len(stored[b]):
                    continue
                got = handle.block(a, r0, nr, b, c0, nc)
                for name in ("binder", "vi", "sumsq"):
                    want = np.ascontiguousarray(getattr(full, name)[r0:r0 + nr, c0:c0 + nc])
                    assert getattr(got, name).tobytes() == want.tobytes(), (a, b, r0, nr, c0, nc, name)
        # one row by many columns and many rows by one column
        row = handle.block(a, 2, 1, b)
        col = handle.block(a, 0, None, b, 1, 1)
        assert row.vi.tobytes() == full.vi[2:3].tobytes() and row.binder.tobytes() == full.binder[2:3].tobytes()
        assert col.vi.tobytes() == np.ascontiguousarray(full.vi[:, 1:2]).tobytes() and col.sumsq.tobytes() == np.ascontiguousarray(full.sumsq[:, 1:2]).tobytes()
        # any output alone gives the bytes it has beside the others
        assert handle.block(a, col_run=b, binder=False, sumsq=False).vi.tobytes() == full.vi.tobytes()
        assert handle.block(a, col_run=b, vi=False, sumsq=False).binder.tobytes() == full.binder.tobytes()
        only = handle.block(a, col_run=b, binder=False, vi=False)
        assert only.sumsq.tobytes() == full.sumsq.tobytes() and only.binder is None and only.vi is None


def test_one_launch_and_one_tile_per_launch_give_the_same_bytes(handle):
    runs = [cases.disjoint(s, 5, 257, seed=7600 + s) for s in (21, 9)]       # K_pad 8: 6 and 3 tiles a side, two rounds of objects
    fill(handle, runs)
    try:
        handle.set_launch_tiles(0)
        whole = {(a, b): handle.block(a, col_run=b) for a in (0, 1) for b in (0, 1)}
        part = handle.block(0, 3, 10, 1, 2, 6)
        sums = handle.sums()
        for tiles in (1, 7):
            handle.set_launch_tiles(tiles)
            for (a, b), want in whole.items():
                same_bytes(handle.block(a, col_run=b), want, f"{tiles} tiles per launch, runs {a} x {b}")
            same_bytes(handle.block(0, 3, 10, 1, 2, 6), part, f"{tiles} tiles per launch, a range")
            got = handle.sums()
            assert got[0].tobytes() == sums[0].tobytes() and got[1].tobytes() == sums[1].tobytes(), tiles
    finally:
        handle.set_launch_tiles(0)
    want_b, want_v = orc.sums(runs)
    same(sums[0], want_b, "binder sums")
    same(sums[1], want_v, "vi sums")


def test_the_largest_number_of_objects_and_the_largest_values():
    """N = 16384, K = 8: all objects in area 0, all in area 1, none clustered, and a split in halves.  The sum of the squared
    sizes reaches 2 N^2 = 2^29 for the first two samples (whose distance is 0: they are one partition); the largest distance
    itself is N^2 = 2^28, between everything in one area and nothing clustered: no two partitions differ in more than all
    N^2 ordered pairs."""
    c = cases.limit()
    n = 16384
    h = partdist.PartitionHandle()
    try:
        h.reset(1, 8, n, 4)
        h.append(0, c)
        got = h.block(0)
        sizes = h.sizes(0)
        tables = h.tables(np.array([(0, x, 0, y) for x in range(4) for y in range(4)], dtype=np.int64)).reshape(4, 4, 8, 8)
    finally:
        h.close()
    assert sizes.tolist() == [[n, 0, 0, 0, 0, 0, 0, 0], [0, n, 0, 0, 0, 0, 0, 0], [0] * 8, [0, 0, n // 2, 0, 0, 0, 0, n // 2]]
    assert int((sizes[0].astype(np.int64) ** 2).sum() + (sizes[1].astype(np.int64) ** 2).sum()) == 1 << 29
    half = n * n // 2
    assert got.binder.tolist() == [[0, 0, 1 << 28, half], [0, 0, 1 << 28, half], [1 << 28, 1 << 28, 0, half], [half, half, half, 0]]
    assert got.sumsq.tolist() == [[n * n, n * n, n * n, half], [n * n, n * n, n * n, half], [n * n, n * n, n * n, half], [half, half, half, half]]
    assert tables[0, 1, 0, 1] == n and tables[0, 3, 0, 2] == n // 2 and tables[3, 3, 7, 7] == n // 2 and tables.sum() == 9 * n
    pos = np.arange(4)
    binder, vi, sumsq = orc.measures(tables, sizes, sizes, n, pos[:, None] > pos[None, :])
    same(got.binder, binder, "binder")
    same(got.vi, vi, "vi")
    same(got.sumsq, sumsq, "sumsq")
    table = orc.xlogx(n)
    h_x, h_y, j = table[n], table[n // 2] + table[n // 2], table[n // 2] + table[n // 2]
    split = ((h_x + h_y) - 2.0 * j) / n                                     # log 2, as the table gives it
    assert got.vi[0, 3] == split and abs(split - np.log(2.0)) <= orc.vi_bound(8, n, h_x + h_y + 2.0 * j)
    assert got.vi[:3, :3].tolist() == [[0.0] * 3] * 3
