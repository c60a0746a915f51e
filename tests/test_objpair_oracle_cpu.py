"""CPU checks of the object-pair check's checker (tests/_objpair_oracle.py): against literal loops on tiny cases, against the
spatial check's checker (tests/_spatial_oracle.py) summed over any classes of pairs, and that the cases of tests/_objpair_cases.py
hold what they claim -- under the checkers alone."""
import numpy as np
import pytest

from tests import _objpair_cases as cases
from tests import _objpair_oracle as orc
from tests import _spatial_oracle as spatial_orc

NA = orc.NA


def literal(y):
    """The contract's definitions, one pair and one cell at a time."""
    n, f_n = y.shape
    agree, comparable = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            for f in range(f_n):
                if y[i, f] != NA and y[j, f] != NA:
                    comparable[i, j] += 1
                    agree[i, j] += int(y[i, f] == y[j, f])
    return agree, comparable


@pytest.mark.parametrize("name", ["n1", "n2", "n31", "n33_f3", "n65_f1"])
def test_the_checker_against_the_literal_loop(name):
    x, _ns, y, want = cases.case(name)
    agree, comparable = literal(x)
    assert np.array_equal(want["agree_obs"], agree) and np.array_equal(want["comparable_obs"], comparable)
    for t in (1, 2, y.shape[0] - 1):
        assert np.array_equal(want["agree_rep"][t], literal(y[t])[0]), t
    # the accumulators, one replicate and one pair at a time
    n = x.shape[0]
    acc = {k: np.zeros((n, n), dtype=np.int64) for k in orc.ACCUMULATORS}
    for t in range(y.shape[0]):
        rep = literal(y[t])[0]
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                v, o = int(rep[i, j]), int(agree[i, j])
                acc["n_greater" if v > o else "n_equal" if v == o else "n_less"][i, j] += 1
                acc["sum"][i, j] += v
                acc["sumsq"][i, j] += v * v
    for k in orc.ACCUMULATORS:
        assert np.array_equal(want[k], acc[k]), k


def test_the_hand_case():
    x, ns, y = cases.hand()
    got = orc.check(x, ns, y)
    assert got["agree_obs"].tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]] and got["comparable_obs"].tolist() == [[0, 2, 3], [2, 0, 2], [3, 2, 0]]
    assert got["agree_rep"][1].tolist() == [[0, 2, 3], [2, 0, 2], [3, 2, 0]] and got["agree_rep"][2].tolist() == [[0, 1, 2], [1, 0, 2], [2, 2, 0]]
    assert got["n_greater"].tolist() == [[0, 0, 1], [0, 0, 2], [1, 2, 0]] and got["n_equal"].tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]
    assert got["n_less"].tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]
    assert got["sum"].tolist() == [[0, 5, 7], [5, 0, 5], [7, 5, 0]] and got["sumsq"].tolist() == [[0, 9, 17], [9, 0, 9], [17, 9, 0]]


@pytest.mark.parametrize("name", ["n2", "n33", "n65", "n97"])
@pytest.mark.parametrize("kind, n_bands", [("quantile", 1), ("quantile", 8), ("knn", 1), ("unequal", 2), ("none", 2)])
def test_the_checker_against_the_spatial_checker(name, kind, n_bands):
    """For any classes of pairs, the pairs' agreements add up to the spatial check's counts: over the pairs of a class to its
    total, over an object's partners in a class to its local_agree -- and the comparable counts likewise."""
    from tests import _spatial_cases as spatial_cases
    x, _ns, y, want = cases.case(name)
    n = x.shape[0]
    rng = np.random.default_rng(7)
    band = spatial_cases.bands(kind, rng.random((n, 2)), n_bands, rng)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    off = ~np.eye(n, dtype=bool)
    for data, agree in ((x, want["agree_obs"]), (y[2], want["agree_rep"][2]), (y[-1], want["agree_rep"][-1])):
        stats = spatial_orc.statistics(data, band, n_bands)
        comparable = orc.statistics(data)[1]
        for b in range(n_bands):
            member = (band == b) & off
            assert int(agree[member & upper].sum()) == int(stats["total"][b])
            assert np.array_equal(np.where(member, agree, 0).sum(axis=1), stats["local_agree"][b])
            assert int(comparable[member & upper].sum()) == int(stats["comparable"][b].sum())
            assert np.array_equal(np.where(member, comparable, 0).sum(axis=1), stats["local_comparable"][b])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_identities_and_the_accumulators(name):
    x, ns, y, want = cases.case(name)
    n, t_n = x.shape[0], y.shape[0]
    off = ~np.eye(n, dtype=bool)
    for k in ("agree_obs", "comparable_obs") + orc.ACCUMULATORS:
        assert np.array_equal(want[k], want[k].T) and not np.diag(want[k]).any(), k
    assert (want["agree_obs"] <= want["comparable_obs"]).all() and (want["comparable_obs"] <= x.shape[1]).all()
    assert ((want["n_greater"] + want["n_equal"] + want["n_less"])[off] == t_n).all() and (want["n_equal"][off] >= 1).all()   # replicate 0 is the data
    again = orc.check(x, ns, np.repeat(x[None], 3, axis=0))                # replicates equal to the data: ties everywhere
    assert (again["n_equal"][off] == 3).all() and not again["n_greater"].any() and not again["n_less"].any()
    assert np.array_equal(again["sum"], 3 * want["agree_obs"].astype(np.int64)) and np.array_equal(again["sumsq"], 3 * want["agree_obs"].astype(np.int64) ** 2)
    none = orc.check(x, ns, y[:0])
    assert none["n_replicates"] == 0 and not any(none[k].any() for k in orc.ACCUMULATORS) and none["agree_rep"].shape == (0, n, n)


def test_the_cases_are_what_they_claim():
    shapes = {name: cases.case(name)[0].shape for name in cases.CASES}
    assert {s[0] for s in shapes.values()} == {1, 2, 31, 32, 33, 64, 65, 97} and {s[1] for s in shapes.values()} == {1, 3, 17}
    assert {orc.elements(cases.case(name)[1])[0] for name in cases.CASES} >= {255, 256, 257, 511, 512, 513}
    assert {orc.elements(cases.case(name)[1])[1] for name in cases.CASES} == {256, 512, 768}     # one, two and three rounds
    for name, (n, f) in shapes.items():
        x, ns, y, want = cases.case(name)
        wanted = cases.CASES[name][3]
        assert wanted is None or orc.elements(ns) == (wanted, -(-wanted // 256) * 256)
        assert ((ns >= 1) & (ns <= 32)).all() and y.shape == (cases.T, n, f) and cases.T == 5
        assert np.array_equal(y[0], x) and ((y == NA) | (y < ns)).all() and ((x == NA) | (x < ns)).all()
        if n > 2:
            assert (x[n // 2] == NA).all() and not want["comparable_obs"][n // 2].any()             # one object all NA
            assert ((y[-1] == NA) & (x != NA)).any()                                                 # the last replicate loses cells
        if f > 2:
            assert (x[:, 1] == NA).all() and ns[-1] == 1 and len(set(ns.tolist())) > (1 if wanted == 513 else 2)     # one feature all NA, one of a single state; mixed (513 = 16 x 32 + 1)
            if n > 2:                                                                                # replicate 2 gains cells
                assert ((y[2] != NA) & (x == NA)).any() and (y[2][:, 1] != NA).any() and (f < 17 or (y[2][n // 2] != NA).any())
    # some pairs agree far more often than others, and the replicates lack that
    x, ns, y, want = cases.case("n97")
    share = want["agree_obs"][np.triu_indices(97, 1)] / np.maximum(1, want["comparable_obs"][np.triu_indices(97, 1)])
    assert np.quantile(share, 0.9) > np.quantile(share, 0.1) + 0.3
    assert (want["n_less"] >= 3).sum() > 100 and (want["n_greater"] >= 3).sum() > 100


def test_the_limit_cases():
    x, ns, y, want = cases.limit("one_state")
    off = ~np.eye(33, dtype=bool)
    assert x.shape == (33, 4096) and (want["agree_obs"][off] == 4096).all() and (want["comparable_obs"][off] == 4096).all()
    assert (want["agree_rep"][:, off] == 4096).all() and (want["n_equal"][off] == 2).all() and (want["sumsq"][off] == 2 * 4096 ** 2).all()
    x, ns, y, want = cases.limit("elements")
    assert orc.elements(ns) == (131072, 131072) and x[x != NA].max() == 31 and (x == NA).any()
    assert 200 < want["agree_obs"][off].min() and want["agree_obs"].max() < 2000 and (want["n_less"][off] + want["n_greater"][off] >= 1).any()


def test_max_replicates_and_replicate_bytes():
    assert orc.max_replicates(1, 1) == orc.max_replicates(4096, 4096) == 2 ** 31 - 1
    assert orc.max_replicates(0, 5) == orc.max_replicates(4097, 1) == orc.max_replicates(5, 4097) == orc.max_replicates(5, 0) == 0
    assert orc.replicate_bytes(1, 1, 1) == 1 + 32 * 128 and orc.replicate_bytes(33, 17, 257, True) == 33 * 17 + 64 * 256 + 4 * 33 * 33
    assert orc.replicate_bytes(1000, 200, 2000) == 200000 + 1024 * 1024 and orc.replicate_bytes(4096, 4096, 131072) == (16 << 20) + (256 << 20)
    assert orc.replicate_bytes(5, 3, 2) == orc.replicate_bytes(5, 3, 97) == orc.replicate_bytes(4097, 3, 3) == 0
