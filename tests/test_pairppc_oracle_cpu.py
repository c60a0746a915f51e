"""CPU checks of the pairwise check's oracle (tests/_pairppc_oracle.py) and cases (tests/_pairppc_cases.py): the observed
statistic is the screening oracle's, the counts and sums are the contract's loop, and every case holds what it claims."""
import numpy as np
import pytest

from sbayes_amd import pairppc
from tests import _assoc_cases as assoc_cases
from tests import _assoc_oracle as ao
from tests import _pairppc_cases as cases
from tests import _pairppc_oracle as orc


@pytest.mark.parametrize("s_pad", [2, 8])
def test_the_observed_statistic_is_the_screening_oracles(s_pad):
    x, ns, want = assoc_cases.sweep(s_pad)
    got = orc.check(x, ns, x[None])
    for ours, theirs in (("stat_obs", "statistic"), ("dof_obs", "dof"), ("n_obs", "n"), ("valid_obs", "valid")):
        assert got[ours].tobytes() == want[theirs].tobytes(), ours
    # the data as its own replicate: every valid pair ties, the sums are the statistic and its square
    v = want["valid"]
    assert np.array_equal(got["n_equal"], v.astype(np.int32)) and not got["n_greater"].any() and not got["n_less"].any()
    assert np.array_equal(got["sum"], want["statistic"]) and np.array_equal(got["sumsq"], want["statistic"] * want["statistic"])


def test_the_planted_tables_of_the_screening_keep_their_statistics():
    _names, x, ns, want = assoc_cases.planted()
    got = orc.check(x, ns, np.stack([x, x]))
    assert got["stat_obs"].tobytes() == want["statistic"].tobytes()
    assert np.array_equal(got["n_equal"], 2 * want["valid"]) and np.array_equal(got["sum"], 2 * want["statistic"])


@pytest.mark.parametrize("name", [n for n in cases.CASES if n not in cases.WIDE])
def test_counts_and_sums_are_the_loop_of_the_contract(name):
    x, ns, y, want = cases.case(name)
    f = x.shape[1]
    for k in orc.INT_FIELDS + ("sum", "sumsq"):
        assert np.array_equal(want[k], want[k].T) and not want[k][~want["valid_obs"]].any(), k
    assert np.array_equal(want["n_greater"] + want["n_equal"] + want["n_less"], cases.T * want["valid_obs"])
    # a direct recomputation, pair by pair, from tables counted here
    for i in range(f):
        for j in range(i + 1, f):
            gt = eq = lt = deg = 0
            total = sq = 0.0
            for t in range(cases.T):
                a, b = y[t, :, i].astype(int), y[t, :, j].astype(int)
                both = (a != orc.NA) & (b != orc.NA)
                table = np.zeros((32, 32), dtype=np.int64)
                np.add.at(table, (a[both], b[both]), 1)
                valid, _dof, _n, s, _r, _c = ao.table_statistic(table)
                if not want["valid_obs"][i, j]:
                    continue
                deg += not valid
                gt, eq, lt = gt + (s > want["stat_obs"][i, j]), eq + (s == want["stat_obs"][i, j]), lt + (s < want["stat_obs"][i, j])
                total += s
                sq += s * s
                assert s == want["stat_rep"][t, i, j]
            assert (gt, eq, lt, deg) == tuple(int(want[k][i, j]) for k in orc.INT_FIELDS), (i, j)
            assert total == want["sum"][i, j] and sq == want["sumsq"][i, j], (i, j)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_cases_are_what_they_claim(name):
    _seed, s_pad, f, n, na_rate, nowhere, one_state = cases.CASES[name]
    x, ns, y, want = cases.case(name)
    t_n = cases.T_WIDE if name in cases.WIDE else cases.T
    assert x.shape == (n, f) and y.shape == (t_n, n, f) and int(ns.max()) == s_pad and len(set(ns.tolist())) > 1
    tiles = -(-f // cases.sub_of(s_pad))
    assert tiles * (tiles + 1) // 2 == {"below_spread": 8128, "at_spread": 8256}.get(name, tiles * (tiles + 1) // 2)
    sub = cases.sub_of(s_pad)
    # more than one tile, a ragged last one (at S_pad = 32 a tile holds one feature: ragged by the last feature's states)
    assert f > sub and (f % sub != 0 or (sub == 1 and ns[-1] < s_pad))
    assert np.array_equal(y == orc.NA, np.broadcast_to(x == orc.NA, y.shape))          # the data's missingness
    assert ((y == orc.NA) | (y < ns[None, None, :])).all()
    share = float((x == orc.NA).mean())
    assert (share == 0.0) if na_rate == 0 and nowhere is None else (0.2 < share < 0.5)
    live = np.triu(want["valid_obs"], 1)
    if n == 1:
        assert not live.any() and not want["stat_rep"].any()
        return
    assert live.sum() >= 3
    if nowhere is not None:
        assert (x[:, nowhere] == orc.NA).all() and not want["valid_obs"][nowhere].any() and not want["n_obs"][nowhere].any()
    if one_state is not None:                                        # observed, but invalid on the data; the replicates vary there
        assert want["n_obs"][one_state].any() and not want["valid_obs"][one_state].any()
        rep = ao.feature_association(y[3], ns)
        assert rep["valid"][one_state].any() and not want["stat_rep"][3][one_state].any()
    # replicate 0 ties everywhere; replicate 2 is degenerate on its feature's pairs and only there
    assert np.array_equal(want["stat_rep"][cases.SAME], want["stat_obs"])
    assert (want["n_equal"][want["valid_obs"]] >= 1).all()
    c = cases.CONSTANT
    assert want["valid_obs"][c].any() and (want["dof_rep"][cases.DEGENERATE][c] == 0).all() and not want["stat_rep"][cases.DEGENERATE][c].any()
    assert np.array_equal(want["n_degenerate"][c] >= 1, want["valid_obs"][c])
    # replicate 1 swaps the labels of a binary feature: the same statistic up to the order of the sum
    s = cases.SWAPPED
    assert ns[s] == 2 and want["valid_obs"][s].any() and (y[cases.SWAP, :, s] != x[:, s])[x[:, s] != orc.NA].all()
    bound = ao.statistic_bound(want["R_obs"], want["C_obs"])[s]
    assert (np.abs(want["stat_rep"][cases.SWAP][s] - want["stat_obs"][s]) <= bound * want["stat_obs"][s]).all()
    # the permuted replicates fall on both sides of dependent pairs, and some replicate is near no tie
    assert want["n_less"].any() and want["n_greater"].any() and orc.near(want).min() == 0 if live.sum() > 5 else True


def test_the_hand_case():
    x, ns, y = cases.hand()
    want = orc.check(x, ns, y)
    assert want["stat_obs"][0, 1] == 4.0 / 1.5 and want["dof_obs"].tolist() == [[0, 1, 2], [1, 0, 2], [2, 2, 0]]
    assert want["n_greater"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]] and want["n_equal"].tolist() == [[0, 2, 3], [2, 0, 2], [3, 2, 0]]
    assert want["n_less"].tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]] and not want["n_degenerate"].any()
    assert want["sum"][1, 2] == 4.0 and want["sumsq"][1, 2] == 16.0 and want["sum"][0, 1] == 2 * want["stat_obs"][0, 1]
    p = orc.p_value(want)
    assert p[0, 1] == 1 / 3 and p[0, 2] == 0.5 and p[1, 2] == 2 / 3


def test_the_result_class_follows_the_oracle():
    x, ns, y, want = cases.case("s8")
    res = pairppc.PairResult(*(want[k] for k in ("stat_obs", "dof_obs", "n_obs", "valid_obs") + orc.INT_FIELDS + ("sum", "sumsq")), cases.T, ns)
    assert np.array_equal(res.p_value(), orc.p_value(want), equal_nan=True)
    v = want["valid_obs"]
    assert np.array_equal(res.mean()[v], (want["sum"] / cases.T)[v]) and np.isnan(res.mean()[~v]).all()
    z, sd = res.z(), res.sd()
    assert np.array_equal(np.isnan(z), ~(sd > 0)) and (sd[v] >= 0).all()
    assert np.allclose(z[sd > 0], ((want["stat_obs"] - res.mean()) / sd)[sd > 0], rtol=0, atol=0)
    flagged = res.flagged(0.5)
    assert flagged == sorted(flagged) and all(i < j and res.p_value()[i, j] < 0.5 for _p, i, j in flagged)
