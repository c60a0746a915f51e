"""The checker of the alignment (tests/_align_oracle.py) against what the reference's own functions returned
(tests/golden/align.npz, recorded by tests/golden/make_align_golden.py) and against SciPy's linear_sum_assignment, the
solver the reference calls.  Under ties SciPy's choice is not part of the contract, so the grid cases are chosen so that
the only tied step is the first (an all-zero matrix, where both give the identity): the comparison leaves no step out."""
from itertools import permutations
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import align
from tests import _align_cases as cases
from tests import _align_oracle as orc

GOLDEN = Path(__file__).resolve().parent / "golden" / "align.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def unpack(g, key, shape_key):
    s, k, n = (int(v) for v in g[shape_key])
    return np.unpackbits(g[key], axis=-1)[:, :, :n].reshape(s, k, n)


def brute(d):
    """(maximum, the lexicographically smallest maximiser) by a plain loop: independent of the checker's solver."""
    k = d.shape[0]
    best, arg = None, None
    for p in permutations(range(k)):                                        # lexicographic order
        v = sum(int(d[i, p[i]]) for i in range(k))
        if best is None or v > best:
            best, arg = v, p
    return best, arg


@pytest.mark.parametrize("n", cases.ORACLE_NS)
@pytest.mark.parametrize("k", cases.ORACLE_KS)
def test_checker_equals_scipy_at_every_step(k, n):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    c, _ = cases.planted(k, n)
    assert c.shape == (cases.S_DEFAULT, k, n)
    perms, ds = orc.within(c, 0, with_d=True)
    nopt = [orc.count_optimal(d) for d in ds]
    assert not ds[0].any() and nopt[0] == len(list(permutations(range(k))))       # the all-zero first step
    assert nopt[1:] == [1] * (len(nopt) - 1), f"K={k} N={n}: tied steps {[i for i, v in enumerate(nopt) if v > 1]}; re-seed the case"
    want = np.array([lsa(d, maximize=True)[1] for d in ds])
    assert np.array_equal(want[0], np.arange(k))
    assert np.array_equal(perms, want)                                      # zero steps excluded
    assert len({tuple(p) for p in perms}) > 1                               # the shuffles are really undone


def test_under_ties_the_checker_takes_the_smallest_maximiser():
    c, _ = cases.planted(5, 33, flip=0.2, seed=80)
    perms, ds = orc.within(c, 0, with_d=True)
    tied = 0
    for p, d in zip(perms, ds):
        best, arg = brute(d)
        assert sum(int(d[i, p[i]]) for i in range(5)) == best
        assert tuple(p) == arg
        tied += orc.count_optimal(d) > 1
    assert tied > 1                                                         # ties beyond the first step do occur here


def test_counter_of_optimal_permutations():
    assert orc.count_optimal(np.zeros((4, 4), dtype=np.int64)) == 24
    assert orc.count_optimal(np.eye(3, dtype=np.int64)) == 1
    assert orc.count_optimal(np.array([[1, 1], [1, 1]])) == 2
    assert orc.best_permutation(np.array([[1, 1], [1, 1]])).tolist() == [0, 1]
    assert orc.best_permutation(np.array([[0, 5, 0], [0, 0, 5], [5, 0, 0]])).tolist() == [1, 2, 0]
    assert orc.best_value(np.array([[0, 5, 0], [0, 0, 5], [5, 0, 0]])) == 15


@pytest.mark.parametrize("tag", ["k3_n100", "k5_n33", "k7_n257"])
def test_logger_sequence_is_reproduced(golden, tag):
    c = unpack(golden, f"logger_{tag}_in", f"logger_{tag}_shape")
    nopt = golden[f"logger_{tag}_nopt"]
    perms, ds = orc.within(c, 0, with_d=True)
    assert [orc.count_optimal(d) for d in ds] == nopt.tolist()
    unique = nopt == 1
    excluded = [s for s in range(len(nopt)) if not unique[s] and ds[s].any()]
    assert excluded == []                                                   # only all-zero steps are tied
    assert np.array_equal(perms[unique], golden[f"logger_{tag}_perms"][unique])
    assert np.array_equal(perms[~unique], np.broadcast_to(np.arange(c.shape[1]), perms[~unique].shape))


@pytest.mark.parametrize("tag", ["k3_n100", "k5_n33"])
def test_realign_tool_is_reproduced_in_the_raw_frame(golden, tag):
    c = unpack(golden, f"realign_{tag}_in", f"realign_{tag}_shape")
    want = unpack(golden, f"realign_{tag}_out", f"realign_{tag}_shape")
    assert (golden[f"realign_{tag}_nopt"] == 1).all()                       # zero steps excluded
    perms = orc.within(c, 20)
    assert np.array_equal(align.apply(c, perms), want)
    assert (perms != np.arange(c.shape[1])).any()
    names = [str(v) for v in golden[f"realign_{tag}_names"]]
    _same, moved = align.permute_stats(names, golden[f"realign_{tag}_params_in"], perms)
    assert np.array_equal(moved, golden[f"realign_{tag}_params_out"])
    assert not np.array_equal(moved, golden[f"realign_{tag}_params_in"])


def test_across_runs_recorded_permutations(golden):
    g = np.load(GOLDEN.parent / "diag_runs.npz")
    kn = int(g["n_cluster_columns"])
    k = 1 + int(str(g["cluster_names"][-1]).split("_")[0][1:])
    runs = [np.unpackbits(g[f"clusters_{r}"], axis=1)[:, :kn].reshape(-1, k, kn // k) for r in range(2)]
    assert int(golden["runs_diag_nopt"]) == 1
    assert np.array_equal(orc.align_runs(runs)["run_perms"][1], golden["runs_diag_perm"])
    k2, n2 = (int(v) for v in golden["runs_planted_shape"])
    planted = [np.unpackbits(golden[f"runs_planted_in{r}"], axis=-1)[:, :, :n2] for r in range(2)]
    assert int(golden["runs_planted_nopt"]) == 1
    got = orc.align_runs(planted)
    assert np.array_equal(got["run_perms"][1], golden["runs_planted_perm"])
    assert np.array_equal(got["run_perms"][0], np.arange(k2))
    relabel = golden["runs_planted_relabel"]                                # row j of run r holds block relabel[r][j]
    assert np.array_equal(relabel[1][got["run_perms"][1]], relabel[0])


@pytest.mark.parametrize("within_seed", [None, 0, 20])
def test_planted_relabellings_are_recovered(within_seed):
    k, n = 4, 100
    relabel = [[0, 1, 2, 3], [3, 1, 0, 2], [1, 2, 3, 0]]
    runs = cases.relabelled_runs(k, n, [40, 33, 48], relabel, seed=900, switch_every=0 if within_seed is None else 5)
    got = orc.align_runs(runs, pivot=0, within_seed=within_seed, burnin=0.1)
    assert np.array_equal(got["run_perms"][0], np.arange(k))
    blocks = [cases.dominant_blocks(k, n, cnt) for cnt in got["counts"]]
    assert len(set(blocks[0])) == k and all(np.array_equal(b, blocks[0]) for b in blocks)
    if within_seed is None:
        for r in range(3):
            assert np.array_equal(np.asarray(relabel[r])[got["run_perms"][r]], relabel[0])
    for r, run in enumerate(runs):                                          # the total permutation is the composition
        aligned = align.apply(align.apply(run, got["perms"][r]), got["run_perms"][r])
        assert np.array_equal(align.apply(run, got["total_perms"][r]), aligned)
        assert np.array_equal(aligned[got["burn_rows"][r]:].sum(axis=0), got["counts"][r])
