"""CPU checks of the spatial check's checker (tests/_spatial_oracle.py): against a literal triple loop on tiny shapes, against
closed forms, and that the cases of tests/_spatial_cases.py hold what they claim -- under the oracle alone."""
from math import comb

import numpy as np
import pytest

from tests import _spatial_cases as cases
from tests import _spatial_oracle as orc

NA = orc.NA


def literal(y, band, n_bands):
    """The contract's definitions, one pair and one cell at a time."""
    n, f_n = y.shape
    agree, comparable = np.zeros((n_bands, f_n), dtype=np.int64), np.zeros((n_bands, f_n), dtype=np.int64)
    local, local_cmp = np.zeros((n_bands, n), dtype=np.int64), np.zeros((n_bands, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            b = int(band[i, j])
            if i == j or b == NA:
                continue
            for f in range(f_n):
                if y[i, f] == NA or y[j, f] == NA:
                    continue
                same = int(y[i, f] == y[j, f])
                local[b, i] += same
                local_cmp[b, i] += 1
                if i < j:
                    agree[b, f] += same
                    comparable[b, f] += 1
    return dict(agree=agree, comparable=comparable, local_agree=local, local_comparable=local_cmp, total=agree.sum(axis=1))


@pytest.mark.parametrize("name", ["n1", "n2", "n63", "n65", "none_counted"])
def test_the_oracle_against_the_literal_loop(name):
    x, _ns, band, b, y, want = cases.case(name)
    for data, suffix, at in ((x, "obs", ()), (y[-1], "rep", (-1,))):
        loop = literal(data, band, b)
        for k in orc.STATS:
            assert np.array_equal(want[f"{k}_{suffix}"][at], loop[k]), (k, suffix)


def test_the_hand_case():
    x, ns, band, b, y = cases.hand()
    got = orc.check(x, ns, band, b, y)
    assert got["agree_obs"].tolist() == [[2, 0], [0, 1]] and got["comparable_obs"].tolist() == [[3, 1], [2, 1]]
    assert got["local_agree_obs"].tolist() == [[1, 1, 1, 1], [1, 0, 1, 0]] and got["total_obs"].tolist() == [2, 1]
    assert got["agree_rep"][1].tolist() == [[3, 0], [2, 1]] and got["total_rep"].tolist() == [[2, 1], [3, 3]]
    assert got["f_greater"].tolist() == [[1, 0], [1, 0]] and got["f_equal"].tolist() == [[1, 2], [1, 2]] and not got["f_less"].any()
    assert got["t_greater"].tolist() == [1, 1] and got["t_equal"].tolist() == [1, 1]
    assert got["f_sum"].tolist() == [[5, 0], [2, 2]] and got["f_sumsq"].tolist() == [[13, 0], [4, 2]]


@pytest.mark.parametrize("n, f", [(1, 1), (2, 3), (7, 2), (65, 3)])
def test_one_state_on_the_complete_graph(n, f):
    x, _ns, band, b = cases.constant(n, f)
    got = orc.statistics(x, band, b)
    assert (got["agree"] == n * (n - 1) // 2).all() and (got["comparable"] == got["agree"]).all()
    assert (got["local_agree"] == (n - 1) * f).all() and got["total"].tolist() == [f * n * (n - 1) // 2]


@pytest.mark.parametrize("n, h", [(2, 1), (9, 4), (64, 1), (65, 32)])
def test_two_halves(n, h):
    x, _ns, band, b = cases.halves(n, h, 2)
    got = orc.statistics(x, band, b)
    assert (got["agree"][0] == comb(h, 2) + comb(n - h, 2)).all() and (got["comparable"][0] == got["agree"][0]).all()
    assert not got["agree"][1].any() and (got["comparable"][1] == h * (n - h)).all()
    assert got["local_agree"][0].tolist() == [2 * (h - 1)] * h + [2 * (n - h - 1)] * (n - h) and not got["local_agree"][1].any()


def test_missing_objects_features_and_classes_count_nowhere():
    x, ns, band, b, y, want = cases.case("n65")
    _seed, _n, _f, _s, _b, _t, _rate, _kind, na_object, na_feature = cases.CASES["n65"]
    assert (x[na_object] == NA).all() and (x[:, na_feature] == NA).all()
    for k in ("agree", "comparable"):
        assert not want[f"{k}_obs"][:, na_feature].any() and not want[f"{k}_rep"][:, :, na_feature].any()
    for k in ("local_agree", "local_comparable"):
        assert not want[f"{k}_obs"][:, na_object].any() and not want[f"{k}_rep"][:, :, na_object].any()
    x, ns, band, b, y, want = cases.case("none_counted")
    assert (band[~np.eye(band.shape[0], dtype=bool)] == NA).all() and (np.diag(band) != NA).any()
    for k in orc.STATS:
        assert not want[f"{k}_obs"].any() and not want[f"{k}_rep"].any()
    assert (want["f_equal"] == y.shape[0]).all() and (want["t_equal"] == y.shape[0]).all()


@pytest.mark.parametrize("name", [n for n in cases.CASES if n not in cases.LARGE])
def test_the_identity_and_the_accumulators(name):
    x, ns, band, b, y, want = cases.case(name)
    t_n = y.shape[0]
    for suffix in ("obs", "rep"):
        assert np.array_equal(want[f"local_agree_{suffix}"].sum(axis=-1), 2 * want[f"total_{suffix}"])
        assert np.array_equal(want[f"local_comparable_{suffix}"].sum(axis=-1), 2 * want[f"comparable_{suffix}"].sum(axis=-1))
        assert (want[f"agree_{suffix}"] <= want[f"comparable_{suffix}"]).all()
    for key in "fit":
        assert (want[f"{key}_greater"] + want[f"{key}_equal"] + want[f"{key}_less"] == t_n).all()
        assert (want[f"{key}_equal"] >= 1).all()                          # replicate 0 is the data
    again = orc.check(x, ns, band, b, np.repeat(x[None], 3, axis=0))       # replicates equal to the data: ties everywhere
    assert all((again[f"{key}_equal"] == 3).all() for key in "fit") and again["n_replicates"] == 3
    assert np.array_equal(again["f_sum"], 3 * want["agree_obs"]) and np.array_equal(again["i_sumsq"], 3 * want["local_agree_obs"] ** 2)


def test_the_cases_are_what_they_claim():
    shapes = {name: cases.case(name)[0].shape for name in cases.CASES if name not in cases.LARGE}
    assert {s[0] for s in shapes.values()} >= {1, 2, 63, 64, 65, 127, 128, 129, 257}
    assert {s[1] for s in shapes.values()} >= {1, cases.TILE - 1, cases.TILE, cases.TILE + 1, 2 * cases.TILE + 1}
    assert {cases.CASES[n][4] for n in cases.CASES} >= {1, 8}
    for name in shapes:
        x, ns, band, b, y, want = cases.case(name)
        assert orc.check_band(band, b) is None and ns[0] == cases.CASES[name][3] and y.shape[0] == cases.CASES[name][5]
        assert np.array_equal(y[0], x) and ((y == NA) | (y < ns)).all()
        if y.shape[0] > 1:
            assert ((y[-1] == NA) & (x != NA)).any() or x.shape[0] < 3    # the last replicate loses cells
    assert {int(cases.case(n)[1].max()) for n in shapes} >= {2, 32}
    # near pairs agree more often than far ones in the data (the geography the replicates lack)
    x, ns, band, b, y, want = cases.case("n257")
    share = want["agree_obs"].sum(axis=1) / want["comparable_obs"].sum(axis=1)
    assert share[0] > share[-1] + 0.05
    assert (want["t_less"][0] >= 1) and want["t_greater"][0] == 0
    # classes of very unequal size
    x, ns, band, b, y, want = cases.case("n128")
    sizes = [int((band[~np.eye(128, dtype=bool)] == k).sum()) for k in range(b)]
    assert sizes[1] > 40 * sizes[0] > 0 and (band == NA).sum() > sizes[1] // 2


def test_the_largest_case():
    x, ns, band, b, y, want = cases.case("n4096")
    assert x.shape == (4096, 3) and y.shape[0] == 2 and orc.check_band(band, b) is None
    assert (want["f_equal"] >= 1).all() and want["total_obs"].min() > 0 and want["agree_obs"].max() > 2 ** 15


def test_band_offences_in_the_contracts_order():
    band = np.full((4, 4), NA, dtype=np.uint8)
    band[0, 1] = band[1, 0] = 1
    assert orc.check_band(band, 2) is None and "band[0][1]=1 is neither below n_bands=1" in orc.check_band(band, 1)
    band[2, 3] = 0                                                        # asymmetric, and a later entry out of range
    band[3, 1] = band[1, 3] = 7
    assert "band[1][3]=7 is neither below" in orc.check_band(band, 2)
    band[3, 1] = band[1, 3] = NA
    assert orc.check_band(band, 2) == "band[2][3]=0 differs from band[3][2]=255"
    band[2, 2] = 200                                                      # the diagonal is ignored
    band[2, 3] = NA
    assert orc.check_band(band, 2) is None


def test_max_replicates():
    assert orc.max_replicates(1, 5) == 2 ** 31 - 1 and orc.max_replicates(0, 5) == orc.max_replicates(4097, 1) == orc.max_replicates(5, 4097) == 0
    assert orc.max_replicates(4096, 4096) == (2 ** 63 - 1) // (4095 * 4096) ** 2 == 32784
    assert orc.max_replicates(4096, 3) == (2 ** 63 - 1) // (4096 * 4095 // 2) ** 2 == 131136
    assert orc.max_replicates(2, 1) == 2 ** 31 - 1 and orc.max_replicates(100, 36) == min(2 ** 31 - 1, (2 ** 63 - 1) // 4950 ** 2)
