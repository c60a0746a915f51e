"""The fp64 restatement of the cost-based geo prior (tests/_geo_oracle.py) against what the reference returned
(tests/golden/geo_prior.npz), against live SciPy on random masks, and its stable log_expit against scipy.special's."""
import numpy as np
import pytest

from tests import _geo_cases as gc
from tests import _geo_oracle as orc


@pytest.fixture(scope="module")
def cases():
    return gc.load()


@pytest.mark.parametrize("name", gc.CASES)
def test_oracle_equals_the_recorded_reference(cases, name):
    c = cases[name]
    sk = gc.oracle_skeletons(c)
    gc.check_skeleton_against_fixture(sk, c, name)
    b = c["masks"].shape[0]
    prior = np.empty((2, 3, 2, b))
    per_object = np.empty((3, 2, b, c["masks"].shape[1]))
    for s, skeleton in enumerate(gc.SKELETONS):
        for a, agg in enumerate(gc.AGGREGATIONS):
            for p, pf in enumerate(gc.PROBABILITY_FUNCTIONS):
                prior[s, a, p] = orc.geo_prior(c["cost"], c["masks"], c["scale"][a], agg, pf, c["x0"][a], skeleton)
                if s == 0:
                    for i, mk in enumerate(c["masks"]):
                        per_object[a, p, i], ctc = orc.costs_per_object(c["cost"], mk, c["scale"][a], agg, pf, c["x0"][a])
                        assert np.array_equal(ctc, c["cost"][mk].min(axis=0))
    gc.check_prior(prior, c["prior"], c, sk, libm=orc.HOST_LIBM, reference_form=True, label=name)
    gc.check_per_object(per_object, c["per_object"], c, sk["mst"], libm=orc.HOST_LIBM, reference_form=True, label=name)


def test_the_cases_are_what_their_names_say(cases):
    sk = {name: gc.oracle_skeletons(cases[name])["mst"] for name in gc.CASES}
    assert np.all(sk["all_zero"]["n_edges"] == 0) and np.all(sk["all_zero"]["sum"] == 0) and np.all(sk["all_zero"]["mean"] == 0)
    assert np.all(sk["single"]["m"] == 1) and np.all(sk["single"]["n_edges"] == 0)
    assert np.all(sk["pair"]["m"] == 2) and sk["pair"]["n_edges"].tolist() == [1, 1, 0]
    assert sk["whole"]["m"].tolist() == [200] and sk["whole"]["n_edges"].tolist() == [199]
    d = sk["duplicates"]                                     # zero-weight tree edges are dropped: the mean is over the rest
    assert np.all(d["n_edges"] < d["m"] - 1) and np.all(d["mean"] * d["n_edges"] == d["sum"])
    assert sorted(sk["synthetic"]["m"].tolist()) == [5, 100, 128, 129, 300]          # both sides of the LDS threshold of 128
    for name in gc.CASES:                                   # the recorded sigmoid arguments stay where both forms agree
        c = cases[name]
        for a, agg in enumerate(gc.AGGREGATIONS):
            for skeleton in gc.SKELETONS:
                x = gc.oracle_skeletons(c)[skeleton][agg]
                assert np.all(-(x - c["x0"][a]) / c["scale"][a] > -700)


@pytest.mark.parametrize("seed,symmetric", [(1, True), (2, True), (3, False)])
def test_oracle_equals_live_scipy_on_random_masks(seed, symmetric):
    pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(seed)
    n = 150
    if symmetric:
        cost = orc.euclidean_cost(rng.uniform(0, 50, size=(n, 2)))
        if seed == 2:
            cost = np.floor(cost / 10)                      # ties and zeros
    else:
        cost = rng.uniform(0.5, 10, size=(n, n))            # both entries of a pair are candidates of one edge
        np.fill_diagonal(cost, 0)
    for size in (1, 2, 3, 17, 60, 150):
        mask = np.zeros(n, dtype=bool)
        mask[rng.choice(n, size=size, replace=False)] = True
        edges = orc.scipy_mst_edges(cost[mask][:, mask])
        got = orc.skeleton(cost, mask, "mst")
        assert max(got["n_edges"], 1) == edges.size and got["max"] == edges.max()
        assert abs(got["sum"] - edges.sum()) <= orc.sum_bound(got["n_edges"]) * edges.sum()
        for agg in gc.AGGREGATIONS:
            for pf in gc.PROBABILITY_FUNCTIONS:
                scale, x0 = 7.0, 20.0
                want = orc.scipy_costs_per_object(cost, mask, scale, agg, pf, x0)
                have, ctc = orc.costs_per_object(cost, mask, scale, agg, pf, x0)
                bound = orc.costs_per_object_bound(ctc, size, got[agg], got["n_edges"], agg, pf, scale, x0, libm=orc.HOST_LIBM)
                assert np.all(np.abs(have - want) <= bound), (size, agg, pf)
                wp = orc.scipy_geo_prior(cost, mask[None], scale, agg, pf, x0)
                hp = orc.geo_prior(cost, mask[None], scale, agg, pf, x0)
                pb = orc.probability_bound(got[agg], orc.aggregate_bound(agg, got["n_edges"]), pf, scale, x0, libm=orc.HOST_LIBM)
                assert np.all(np.abs(hp - wp) <= pb), (size, agg, pf)


def test_stable_log_expit_against_scipy_where_the_reference_form_diverges():
    special = pytest.importorskip("scipy.special")
    t = np.concatenate([np.linspace(-2000, 50, 4101), [-745.2, -744.0, -709.9, -700.0, -40.0, -1e-300, 0.0, 1e-300, 36.8, 745.0]])
    want = special.log_expit(t)
    got = orc.log_expit(t)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= orc.HOST_LIBM * np.abs(want))
    with np.errstate(divide="ignore"):
        reference_form = np.log(special.expit(t))           # what the reference runs under SciPy 1.15
    assert np.all(np.isneginf(reference_form[t < -746])) and np.all(got[t < -746] == t[t < -746])
    agree = t > -700                                         # above: the two forms agree to expit's rounding
    assert np.all(np.abs(reference_form[agree] - got[agree]) <= orc.HOST_LIBM * np.abs(got[agree]) + 2 * orc.U)
    # the sigmoid of an aggregate far beyond the inflection point: finite in the stable form
    assert np.isfinite(orc.probability(1e6, "sigmoid", 1.0, 10.0)) and orc.probability(1e6, "sigmoid", 1.0, 10.0) < -9e5
